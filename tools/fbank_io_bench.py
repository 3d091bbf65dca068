#!/usr/bin/env python3
"""Kaldi fbank: int16 PCM in / f16 features out against the f32 call and against the status quo, in one process on one GPU
(profiles/fbank_io_dtypes.txt).  The sibling of tools/blm_io_bench.py.

Shape: BASELINE config 3 -- 1024 x 10 s, 80 bins, CMN on, noise.  Variants, timed with device events over --rounds rounds of --calls calls
after a warm-up; a round times every variant once, even rounds in the order A B D, odd rounds in the reverse order:
  A  the existing f32 call (this batch: fbank512_clip_kernel, the CMN inside)
  B  the status quo of a caller who holds int16 and wants f16: pcm16.to(float32).mul_(2**-15), call A, .to(float16) -- all on the device,
     all inside the timed window, on the same stream
  D  (S16, F16) through melspec_fbank_compute_uniform_device_io (the wave-owned kernel into the f32 scratch, then cmn_io_kernel)
Per variant: the median of the rounds and their spread (max - min), frames per second, and the fraction of the HBM peak that the call's OWN
algorithmic bytes per frame amount to at that time (160 samples in, 80 features out: A 640 + 320 B, B the same + the two casts' 320 + 640
and 320 + 160, D 320 + 160 B).  The claim to confirm or refute: D faster than B; D is not expected to beat A.

  python tools/fbank_io_bench.py [--out profiles/fbank_io_dtypes.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0   # bench.py


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_io_dtypes.txt"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd.hip import OUT_F16, PCM_S16
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n_clips, n, nm = 1024, 160000, 80
    gen = torch.Generator(device=dev).manual_seed(4321)
    pcm16 = torch.randint(-32768, 32768, (n_clips, n), generator=gen, device=dev, dtype=torch.int32)
    pcm16 = (pcm16 >> (torch.arange(n_clips, device=dev, dtype=torch.int32) & 7)[:, None]).to(torch.int16).contiguous()
    pcm32 = pcm16.to(torch.float32).mul_(2.0 ** -15)
    fb = M.Fbank(M.FbankConfig(), device=0)
    assert fb.uses_fast_path and fb.supports_io(PCM_S16, OUT_F16)
    nf = fb.num_frames(n)
    frames = n_clips * nf
    out32 = torch.empty((n_clips, nf, nm), device=dev, dtype=torch.float32)
    out16 = torch.empty((n_clips, nf, nm), device=dev, dtype=torch.int16)

    def call_a(src=None):
        fb.compute_uniform_device((pcm32 if src is None else src).data_ptr(), n, n, n_clips, out32.data_ptr(), stream)

    def call_b():
        call_a(pcm16.to(torch.float32).mul_(2.0 ** -15))
        return out32.to(torch.float16)

    def call_d():
        fb.compute_uniform_device_io(pcm16.data_ptr(), PCM_S16, n, n, n_clips, out16.data_ptr(), OUT_F16, stream)

    variants = [("A", call_a), ("B", call_b), ("D", call_d)]
    call_d()
    want = call_b()
    torch.cuda.synchronize()
    assert torch.equal(out16.view(torch.float16), want), "D != the status quo's result"       # bit for bit, before anything is timed
    for _, fn in variants:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in variants}
    for r in range(args.rounds):
        for label, fn in (variants if r % 2 == 0 else variants[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            ms[label].append(e0.elapsed_time(e1) / args.calls)
    bytes_per_frame = {"A": 640 + 320, "B": (320 + 640) + (640 + 320) + (320 + 160), "D": 320 + 160}
    what = {"A": "the f32 call", "B": "status quo: to(f32) * 2^-15, A, to(f16)", "D": "(S16, F16) through the _io call"}
    lines = [f"# tools/fbank_io_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# config 3: {n_clips} x 10 s, 80 bins, CMN on ({frames} frames); {args.rounds} rounds x {args.calls} calls per variant, order A B D and its reverse in turn, "
             f"after {args.warmup} warm-up calls each; device events",
             f"# HBM fraction: the call's own algorithmic bytes per frame at the measured time against {HBM_PEAK_GBS:.0f} GB/s",
             f"# {'':1s} {'ms / call':>9s} {'spread':>7s} {'frames / s':>11s} {'B / frame':>9s} {'of HBM peak':>11s}"]
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k, _ in variants:
        gbs = bytes_per_frame[k] * frames / (med[k] * 1e-3) / 1e9
        lines.append(f"  {k} {med[k]:9.4f} {max(ms[k]) - min(ms[k]):7.4f} {frames / (med[k] * 1e-3):11.4e} {bytes_per_frame[k]:9d} {gbs / HBM_PEAK_GBS:11.4f}   {what[k]}")
    lines.append(f"# B / D = {med['B'] / med['D']:.2f}, D / A = {med['D'] / med['A']:.2f}: D is " + ("faster than B" if med["D"] < med["B"] else "NOT faster than B") +
                 ", " + ("faster than A" if med["D"] < med["A"] else "slower than A"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)
    fb.close()


if __name__ == "__main__":
    main()
