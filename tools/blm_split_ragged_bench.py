#!/usr/bin/env python3
"""NeMo / Parakeet frontend, ragged batches: the split output (melspec_blm_compute_ragged_device_split: rows + per-feature mean and
1 / std from the mel kernel) against the raw ragged call and against the normalised ragged call it replaces, in one process on one GPU
(profiles/blm_split_ragged.txt).

Shape: 1024 clips of noise, lengths drawn (seeded) uniformly from 2 s to 20 s, at 80 and 128 mels, default (f64) and
MELSPEC_PRECISION_F32 arithmetic.  Variants:
  A  melspec_blm_compute_ragged_device_split: the ragged stats kernel + blm_stats_finish_ragged_kernel
  B  melspec_blm_compute_ragged_device of a normalize_per_feature = 0 context: the mel kernel alone
  C  melspec_blm_compute_ragged_device of a normalize_per_feature = 1 context: the mel kernel + blm_normalize_ragged_kernel -- the call A
     replaces; its kernels are the parent commit's, instruction for instruction
Every timed call is one call followed by a synchronise of its stream, timed with the host clock: a ragged call plans its batch on the
host and sends the plan up, and that is part of what a caller pays.  After a warm-up of every variant a round times each variant once,
even rounds in the order A B C, odd rounds in reverse; per variant the median of the rounds and their spread (max - min).

  python tools/blm_split_ragged_bench.py [--out profiles/blm_split_ragged.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blm_split_ragged.txt"))
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--clips", type=int, default=1024)
    args = ap.parse_args()
    assert args.rounds >= 20, "the median of at least 20 timed calls"

    import numpy as np
    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no other way to run it"
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lens = np.random.default_rng(2020).integers(2 * 16000, 20 * 16000 + 1, args.clips).astype(np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    total = int(lens.sum())
    gen = torch.Generator(device=dev).manual_seed(4321)
    pcm = torch.randn((total,), generator=gen, device=dev, dtype=torch.float32).mul_(0.1)

    lines = [f"# tools/blm_split_ragged_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {args.clips} clips of noise, 2 s .. 20 s (seeded), {total / 16000:.0f} s in all; {args.rounds} rounds, a round = one call of each variant ending in a synchronise "
             f"(host clock), order A B C and its reverse in turn, after {args.warmup} warm-up calls each; ms per call, median of the rounds",
             "# A the ragged split call (stats kernel + finisher); B the raw ragged call (normalize_per_feature = 0); C the normalised ragged call (mel kernel + blm_normalize_ragged_kernel)",
             f"# {'mels':>4s} {'mode':>4s} | {'A':>8s} {'B':>8s} {'C':>8s} | {'spread':>7s} | {'A / B':>6s} {'A / C':>6s} {'A - B':>8s} {'C - A':>8s}  verdict"]
    for nm in (80, 128):
        for mode in ("f64", "f32"):
            raw = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=False), device=0)
            norm = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=True), device=0)
            for fe in (raw, norm):
                fe.set_precision(mode)
                assert fe.precision == mode
            assert raw.supports_split()
            cols = np.array([raw.padded_frames(int(n)) for n in lens], np.int64)
            floats = int(cols.sum()) * nm
            bufs = {k: torch.empty((floats,), device=dev, dtype=torch.float32) for k in "ABC"}
            mean = torch.empty((args.clips, nm), device=dev, dtype=torch.float32)
            inv_std = torch.empty((args.clips, nm), device=dev, dtype=torch.float32)

            def timed(fe, fn):
                def run():
                    t0 = time.perf_counter()
                    fn()
                    fe.synchronize(stream)
                    return (time.perf_counter() - t0) * 1e3
                return run
            variants = [
                ("A", timed(raw, lambda: M.blm_compute_ragged_device_split(raw, pcm.data_ptr(), offs, lens, bufs["A"].data_ptr(), mean.data_ptr(), inv_std.data_ptr(), None, stream))),
                ("B", timed(raw, lambda: raw.compute_ragged_device(pcm.data_ptr(), offs, lens, bufs["B"].data_ptr(), None, stream))),
                ("C", timed(norm, lambda: norm.compute_ragged_device(pcm.data_ptr(), offs, lens, bufs["C"].data_ptr(), None, stream))),
            ]
            # before anything is timed: A's rows are B's bits, and the consumer's (x - mean) * inv_std is C's output to f32 rounding
            for _, fn in variants:
                fn()
            torch.cuda.synchronize()
            assert torch.equal(bufs["A"].view(torch.int32), bufs["B"].view(torch.int32)), "A's rows are not the raw call's bits"
            worst, at = 0.0, 0
            for c in range(4):
                valid, w = raw.num_frames(int(lens[c])), int(cols[c])
                a = bufs["A"][at:at + nm * w].view(nm, w)[:, :valid]
                z = (a - mean[c, :, None]) * inv_std[c, :, None]
                worst = max(worst, float((z - bufs["C"][at:at + nm * w].view(nm, w)[:, :valid]).abs().max()))
                at += nm * w
            assert worst < 1e-3, worst
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
            verdict = ("A below C" if med["A"] + iqr < med["C"] else "A NOT clearly below C") + ", " + \
                      ("A within the quartiles of B" if abs(med["A"] - med["B"]) <= iqr else f"A {'above' if med['A'] > med['B'] else 'below'} B by {abs(med['A'] / med['B'] - 1) * 100:.1f} %")
            lines.append(f"  {nm:4d} {mode:>4s} | {med['A']:8.4f} {med['B']:8.4f} {med['C']:8.4f} | {spread:7.4f} | {med['A'] / med['B']:6.3f} {med['A'] / med['C']:6.3f} "
                         f"{med['A'] - med['B']:+8.4f} {med['C'] - med['A']:+8.4f}  {verdict}   (widest interquartile range {iqr:.4f}; |z - C| on four clips: {worst:.1e})")
            print(lines[-1], flush=True)
            for fe in (raw, norm):
                fe.close()
            del bufs, mean, inv_std
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
