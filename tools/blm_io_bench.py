#!/usr/bin/env python3
"""NeMo / Parakeet frontend: int16 PCM in / f16, bf16 features out against the f32 call and against the status quo, in one process on one
GPU (profiles/blm_io_dtypes.txt).  The sibling of tools/io_bench.py.

Shape: 1024 x 10 s at 80 and 128 mels, normalize_per_feature off and on, default (f64) and MELSPEC_PRECISION_F32 arithmetic, noise.
Variants, timed with device events over --rounds rounds of --calls calls after a warm-up; a round times every variant once, even rounds in
the order A Sh Sb D E, odd rounds in the reverse order:
  A   the existing f32 call                                    D  (S16, F16)      E  (S16, BF16)
  Sh  the status quo of a caller who holds int16 and wants f16: pcm16.to(float32).mul_(2**-15), call A, .to(float16) -- all on the
      device, all inside the timed window, on the same stream
  Sb  the same for bf16: ... .to(bfloat16)
Per variant: the median of the rounds and their spread (max - min).  The claim to confirm or refute per row: D faster than Sh, E faster
than Sb, and neither slower than A.

--ragged: instead, the ragged normaliser (blm_normalize_ragged_kernel / blm_normalize_ragged_io_kernel): 1024 clips of 5..15 s in one ragged
call, normalize_per_feature on, 80 and 128 mels; A the f32 ragged call, D (S16, F16), E (S16, BF16); same rounds, medians and spread.

  python tools/blm_io_bench.py [--ragged] [--out profiles/blm_io_dtypes.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blm_io_dtypes.txt"))
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ragged", action="store_true")
    args = ap.parse_args()

    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd.hip import OUT_BF16, OUT_F16, PCM_S16
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n_clips, n = 1024, 160000
    lines = [f"# tools/blm_io_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {n_clips} x 10 s; {args.rounds} rounds x {args.calls} calls per variant, order A Sh Sb D E and its reverse in turn, after {args.warmup} warm-up calls each; device events; ms per call",
             "# A the f32 call; Sh / Sb the status quo: to(f32) * 2^-15, A, to(f16) / to(bf16); D (S16, F16); E (S16, BF16)",
             f"# {'mels':>4s} {'mode':>4s} {'norm':>4s} | {'A':>8s} {'Sh':>8s} {'Sb':>8s} {'D':>8s} {'E':>8s} | {'spread':>7s} | {'Sh / D':>6s} {'Sb / E':>6s} {'D - A':>8s} {'E - A':>8s}  verdict"]
    gen = torch.Generator(device=dev).manual_seed(4321)
    pcm16 = torch.randint(-32768, 32768, (n_clips, n), generator=gen, device=dev, dtype=torch.int32)
    pcm16 = (pcm16 >> (torch.arange(n_clips, device=dev, dtype=torch.int32) & 7)[:, None]).to(torch.int16).contiguous()
    pcm32 = pcm16.to(torch.float32).mul_(2.0 ** -15)
    if args.ragged:
        return ragged(args, torch, M, (PCM_S16, OUT_F16, OUT_BF16), pcm16, pcm32, stream, lines[:1])
    for nm in (80, 128):
        for mode in ("f64", "f32"):
            for norm in (False, True):
                fe = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=norm), device=0)
                fe.set_precision(mode)
                assert fe.precision == mode
                cols = fe.padded_frames(n)
                out32 = torch.empty((n_clips, nm, cols), device=dev, dtype=torch.float32)
                out16 = torch.empty((n_clips, nm, cols), device=dev, dtype=torch.int16)

                def call_a(src=None):
                    fe.compute_uniform_device((pcm32 if src is None else src).data_ptr(), n, n, n_clips, out32.data_ptr(), stream)

                def status_quo(dt):
                    def run():
                        call_a(pcm16.to(torch.float32).mul_(2.0 ** -15))
                        return out32.to(dt)
                    return run

                def io(out):
                    return lambda: fe.compute_uniform_device_io(pcm16.data_ptr(), PCM_S16, n, n, n_clips, out16.data_ptr(), out, stream)

                variants = [("A", call_a), ("Sh", status_quo(torch.float16)), ("Sb", status_quo(torch.bfloat16)), ("D", io(OUT_F16)), ("E", io(OUT_BF16))]
                for label, quo, dt in (("D", "Sh", torch.float16), ("E", "Sb", torch.bfloat16)):     # == the status quo's result, bit for bit, before anything is timed
                    dict(variants)[label]()
                    want = dict(variants)[quo]()
                    torch.cuda.synchronize()
                    assert torch.equal(out16.view(dt), want), f"{label} != the status quo's result"
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
                med = {k: statistics.median(v) for k, v in ms.items()}
                spread = max(max(v) - min(v) for v in ms.values())
                worst16 = max(med["D"], med["E"])
                verdict = ("faster than S" if med["D"] < med["Sh"] and med["E"] < med["Sb"] else "NOT faster than S") + ", " + \
                          ("faster than A" if worst16 < med["A"] else "within the spread of A" if worst16 - med["A"] <= spread else "SLOWER than A beyond the spread")
                lines.append(f"  {nm:4d} {mode:>4s} {int(norm):4d} | {med['A']:8.4f} {med['Sh']:8.4f} {med['Sb']:8.4f} {med['D']:8.4f} {med['E']:8.4f} | {spread:7.4f} | "
                             f"{med['Sh'] / med['D']:6.2f} {med['Sb'] / med['E']:6.2f} {med['D'] - med['A']:+8.4f} {med['E'] - med['A']:+8.4f}  {verdict}")
                print(lines[-1], flush=True)
                fe.close()
                del out32, out16
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)


def ragged(args, torch, M, codes, pcm16, pcm32, stream, lines):
    import numpy as np
    pcm_s16, out_f16, out_bf16 = codes
    from mel_spec_amd.hip import OUT_F32, PCM_F32        # (F32, F32) through the _io call is the f32 call
    n_clips, n = pcm16.shape
    lengths = np.random.default_rng(7).integers(80000, 240001, n_clips).astype(np.uint64)      # 5 .. 15 s
    offsets = np.zeros(n_clips, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)[:-1]
    flat16 = torch.cat([pcm16.reshape(-1), pcm16.reshape(-1)[: int(lengths.sum()) - pcm16.numel()]]) if int(lengths.sum()) > pcm16.numel() else pcm16.reshape(-1)
    flat32 = flat16.to(torch.float32).mul_(2.0 ** -15)
    lines += [f"# --ragged: {n_clips} clips of 5..15 s ({int(lengths.sum()) / 16000:.0f} s) in one ragged call, normalize_per_feature on; {args.rounds} rounds x {args.calls} calls per variant, "
              f"order A D E and its reverse in turn, after {args.warmup} warm-up calls each; device events; ms per call",
              "# A the f32 ragged call (in place); D (S16, F16); E (S16, BF16): blm_normalize_ragged_io_kernel from the scratch",
              f"# {'mels':>4s} | {'A':>8s} {'D':>8s} {'E':>8s} | {'spread':>7s}"]
    for nm in (80, 128):
        fe = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=True), device=0)
        total = sum(fe.padded_frames(int(x)) for x in lengths) * nm
        out32 = torch.empty(total, device=flat16.device, dtype=torch.float32)
        out16 = torch.empty(total, device=flat16.device, dtype=torch.int16)
        variants = [("A", lambda: fe.compute_ragged_device_io(flat32.data_ptr(), PCM_F32, offsets, lengths, out32.data_ptr(), OUT_F32, None, stream)),
                    ("D", lambda: fe.compute_ragged_device_io(flat16.data_ptr(), pcm_s16, offsets, lengths, out16.data_ptr(), out_f16, None, stream)),
                    ("E", lambda: fe.compute_ragged_device_io(flat16.data_ptr(), pcm_s16, offsets, lengths, out16.data_ptr(), out_bf16, None, stream))]
        variants[0][1](); variants[1][1]()
        torch.cuda.synchronize()
        assert torch.equal(out16.view(torch.float16), out32.to(torch.float16)), "D != the f32 call's rows rounded once"
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
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        lines.append(f"  {nm:4d} | {med['A']:8.4f} {med['D']:8.4f} {med['E']:8.4f} | {spread:7.4f}")
        print(lines[-1], flush=True)
        fe.close()
        del out32, out16
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
