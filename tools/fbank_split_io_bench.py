#!/usr/bin/env python3
"""Kaldi fbank: the split output with 16-bit ends (melspec_fbank_compute_{uniform,ragged}_device_split_io: int16 PCM in, f16 rows out,
f32 means, one pass of the workgroup-per-clip kernel) against what a caller had before it, in one process on one GPU
(profiles/fbank_split_io.txt).  The sibling of tools/blm_split_io_bench.py and tools/fbank_io_bench.py.

Shapes: BASELINE config 3 -- 1024 clips of 10 s (uniform call) -- and 1024 clips of noise with lengths drawn (seeded) uniformly from 2 s
to 20 s (ragged call); 80 bins, CMN on.  Variants:
  A  the new call, (S16, F16): fbank512_clip_split_io_kernel; no scratch rows, no second pass
  B  melspec_fbank_compute_*_device_io (S16, F16) with CMN: the wave kernel writes f32 rows into the object's scratch, cmn_io_kernel reads
     them and writes f16 -- the call A replaces for a consumer that folds the subtraction into its own first read; the parent commit's kernels
  C  the f32 split on f32 samples: melspec_fbank_compute_uniform_device_split (existing) / melspec_fbank_compute_ragged_device_split (new)
  D  the status quo built from parts: torch int16 -> f32 (times 2^-15), C, torch f32 -> f16 of the rows
Every timed call is one call followed by a synchronise of its stream, timed with the host clock (a ragged call plans its batch on the
host and sends the plan up: part of what a caller pays).  After a warm-up of every variant a round times each variant once, even rounds
in the order A B C D, odd rounds in reverse; per variant the median of the rounds, the spread (max - min) and the widest interquartile
range.

  python tools/fbank_split_io_bench.py [--out profiles/fbank_split_io.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_split_io.txt"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=1024)
    args = ap.parse_args()
    assert args.rounds >= 20, "the median of at least 20 timed calls"

    import numpy as np
    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd.hip import OUT_F16, PCM_S16
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no other way to run it"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    gen = torch.Generator(device=dev).manual_seed(4321)
    nm = 80

    def batch(shape):
        if shape == "uniform":
            lens = np.full(args.clips, 160000, np.uint64)
        else:
            lens = np.random.default_rng(2020).integers(2 * 16000, 20 * 16000 + 1, args.clips).astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        total = int(lens.sum())
        s16 = torch.randn((total,), generator=gen, device=dev, dtype=torch.float32).mul_(0.1 * 32768.0).round_().clamp_(-32768, 32767).to(torch.int16)
        return lens, offs, total, s16

    lines = [f"# tools/fbank_split_io_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {args.clips} clips of int16 noise, 80 bins, CMN on: uniform = 10 s each (config 3), ragged = 2 s .. 20 s (seeded); {args.rounds} rounds, a round = one call of "
             f"each variant ending in a synchronise (host clock), order A B C D and its reverse in turn, after {args.warmup} warm-up calls each; ms per call, median of the rounds",
             "# A the split call (S16, F16); B the _io call (S16, F16) with CMN, which A replaces; C the f32 split on f32 samples; D torch int16 -> f32, C, torch f32 -> f16",
             f"# {'shape':>7s} | {'A':>8s} {'B':>8s} {'C':>8s} {'D':>8s} | {'spread':>7s} {'iqr':>7s} | {'A / B':>6s} {'A / C':>6s} {'A / D':>6s}  verdict"]
    for shape in ("uniform", "ragged"):
        lens, offs, total, s16 = batch(shape)
        pcm32 = s16.to(torch.float32).mul_(2.0 ** -15)
        fb = M.Fbank(M.FbankConfig(), device=0)
        assert fb.uses_fast_path and M.fbank_supports_split_io(fb, PCM_S16, OUT_F16) and fb.supports_io(PCM_S16, OUT_F16)
        frames = np.array([fb.num_frames(int(n)) for n in lens], np.int64)
        elems = int(frames.sum()) * nm
        rows16 = {k: torch.empty((elems,), device=dev, dtype=torch.float16) for k in "AB"}
        rows32 = torch.empty((elems,), device=dev, dtype=torch.float32)
        means = {k: torch.empty((args.clips, nm), device=dev, dtype=torch.float32) for k in "AC"}
        kept = {}
        n0 = int(lens[0])

        def a():
            if shape == "uniform":
                M.fbank_compute_uniform_device_split_io(fb, s16.data_ptr(), PCM_S16, n0, n0, args.clips, rows16["A"].data_ptr(), OUT_F16, means["A"].data_ptr(), stream)
            else:
                M.fbank_compute_ragged_device_split_io(fb, s16.data_ptr(), PCM_S16, offs, lens, rows16["A"].data_ptr(), OUT_F16, means["A"].data_ptr(), None, stream)

        def b():
            if shape == "uniform":
                fb.compute_uniform_device_io(s16.data_ptr(), PCM_S16, n0, n0, args.clips, rows16["B"].data_ptr(), OUT_F16, stream)
            else:
                fb.compute_ragged_device_io(s16.data_ptr(), PCM_S16, offs, lens, rows16["B"].data_ptr(), OUT_F16, None, stream)

        def c(src=None):
            p = pcm32 if src is None else src
            if shape == "uniform":
                fb.compute_uniform_device_split(p.data_ptr(), n0, n0, args.clips, rows32.data_ptr(), means["C"].data_ptr(), stream)
            else:
                M.fbank_compute_ragged_device_split(fb, p.data_ptr(), offs, lens, rows32.data_ptr(), means["C"].data_ptr(), None, stream)

        def d():
            x = s16.to(torch.float32).mul_(2.0 ** -15)
            c(x)
            kept["D"] = rows32.to(torch.float16)

        def timed(fn):
            def run():
                t0 = time.perf_counter()
                fn()
                fb.synchronize(stream)
                return (time.perf_counter() - t0) * 1e3
            return run
        variants = [("A", timed(a)), ("B", timed(b)), ("C", timed(c)), ("D", timed(d))]
        # before anything is timed: A's rows are D's bits and its means C's, and the consumer's x - mean is B's output to the rounding of the
        # f16 rows
        for _, fn in variants:
            fn()
        torch.cuda.synchronize()
        assert torch.equal(rows16["A"].view(torch.int16), kept["D"].view(torch.int16)), "A's rows are not the f32 split's, rounded"
        assert torch.equal(means["A"].view(torch.int32), means["C"].view(torch.int32)), "A's means are not the f32 split's bits"
        worst, at = 0.0, 0
        for k in range(4):
            f = int(frames[k])
            z = rows16["A"][at:at + f * nm].view(f, nm).float() - means["A"][k][None, :]
            worst = max(worst, float((z - rows16["B"][at:at + f * nm].view(f, nm).float()).abs().max()))
            at += f * nm
        assert worst < 0.05, worst           # a sanity check: an ulp of f16 at |x| < 32 is 2^-6
        for _, fn in variants:
            for _ in range(args.warmup):
                fn()
        ms = {k: [] for k, _ in variants}
        for r in range(args.rounds):
            for label, fn in (variants if r % 2 == 0 else variants[::-1]):
                ms[label].append(fn())
        med = {k: statistics.median(v) for k, v in ms.items()}
        spread = max(max(v) - min(v) for v in ms.values())
        iqr = max(statistics.quantiles(v, n=4)[2] - statistics.quantiles(v, n=4)[0] for v in ms.values())
        verdict = ", ".join(f"A below {k}" if med["A"] + iqr < med[k] else f"A NOT clearly below {k}" for k in "BCD")
        lines.append(f"  {shape:>7s} | {med['A']:8.4f} {med['B']:8.4f} {med['C']:8.4f} {med['D']:8.4f} | {spread:7.4f} {iqr:7.4f} | "
                     f"{med['A'] / med['B']:6.3f} {med['A'] / med['C']:6.3f} {med['A'] / med['D']:6.3f}  {verdict}   (|A - mean - B| on four clips: {worst:.1e})")
        print(lines[-1], flush=True)
        fb.close()
        del rows16, rows32, means, kept, s16, pcm32
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
