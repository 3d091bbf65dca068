#!/usr/bin/env python3
"""NeMo / Parakeet frontend: the split output (rows + per-feature mean and 1 / std from the mel kernel) against the raw call and against
the normalised call, in one process on one GPU (profiles/blm_split.txt).

Shape: 1024 x 10 s of noise at 80 and 128 mels, default (f64) and MELSPEC_PRECISION_F32 arithmetic.  Variants, timed with device events over
--rounds rounds of --calls calls after a warm-up; a round times every variant once, even rounds in the order A B C, odd rounds in reverse:
  A  melspec_blm_compute_uniform_device_split: the stats kernel + blm_stats_finish_kernel
  B  melspec_blm_compute_uniform_device of a normalize_per_feature = 0 context: the mel kernel alone
  C  melspec_blm_compute_uniform_device of a normalize_per_feature = 1 context: the mel kernel + blm_normalize_kernel (what a caller who
     wants normalised features pays today; the kernels of this call are the parent commit's, instruction for instruction)
Per variant: the median of the rounds and their spread (max - min).  The aims: A costs what B costs plus the partial stores and the
finisher, and clearly less than C.

Timing only.  A mode of this tool for a FETCH_SIZE / WRITE_SIZE counter run was taken out again: the one attempt aborted under the
profiler before any kernel of the library had run, its cause was not found, and nothing here invites a second one.

  python tools/blm_split_bench.py [--out profiles/blm_split.txt]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def variants_for(torch, M, nm, mode, pcm, stream):
    n_clips, n = pcm.shape
    dev = pcm.device
    raw = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=False), device=0)
    norm = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=True), device=0)
    for fe in (raw, norm):
        fe.set_precision(mode)
        assert fe.precision == mode
    assert raw.supports_split()
    cols = raw.padded_frames(n)
    bufs = {k: torch.empty((n_clips, nm, cols), device=dev, dtype=torch.float32) for k in "ABC"}
    mean = torch.empty((n_clips, nm), device=dev, dtype=torch.float32)
    inv_std = torch.empty((n_clips, nm), device=dev, dtype=torch.float32)
    calls = {
        "A": lambda: raw.compute_uniform_device_split(pcm.data_ptr(), n, n, n_clips, bufs["A"].data_ptr(), mean.data_ptr(), inv_std.data_ptr(), stream),
        "B": lambda: raw.compute_uniform_device(pcm.data_ptr(), n, n, n_clips, bufs["B"].data_ptr(), stream),
        "C": lambda: norm.compute_uniform_device(pcm.data_ptr(), n, n, n_clips, bufs["C"].data_ptr(), stream),
    }
    return calls, bufs, mean, inv_std, (raw, norm), raw.num_frames(n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blm_split.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()

    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    n_clips, n = 1024, 160000
    gen = torch.Generator(device=dev).manual_seed(4321)
    pcm = torch.randn((n_clips, n), generator=gen, device=dev, dtype=torch.float32).mul_(0.1)

    lines = [f"# tools/blm_split_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {n_clips} x 10 s of noise; {args.rounds} rounds x {args.calls} calls per variant, order A B C and its reverse in turn, after {args.warmup} warm-up calls each; "
             "device events; ms per call, median of the rounds",
             "# A the split call (stats kernel + finisher); B the raw call (normalize_per_feature = 0); C the normalised call (mel kernel + blm_normalize_kernel)",
             f"# {'mels':>4s} {'mode':>4s} | {'A':>8s} {'B':>8s} {'C':>8s} | {'spread':>7s} | {'A / B':>6s} {'A / C':>6s} {'A - B':>8s} {'C - A':>8s}  verdict"]
    for nm in (80, 128):
        for mode in ("f64", "f32"):
            calls, bufs, mean, inv_std, fes, valid = variants_for(torch, M, nm, mode, pcm, stream)
            variants = [(k, calls[k]) for k in "ABC"]
            # before anything is timed: A's rows are B's bits, and the consumer's (x - mean) * inv_std is C's output to f32 rounding
            for _, fn in variants:
                fn()
            torch.cuda.synchronize()
            assert torch.equal(bufs["A"].view(torch.int32), bufs["B"].view(torch.int32)), "A's rows are not the raw call's bits"
            z = (bufs["A"][:4, :, :valid] - mean[:4, :, None]) * inv_std[:4, :, None]
            worst = float((z - bufs["C"][:4, :, :valid]).abs().max())
            assert worst < 1e-3, worst
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
            verdict = ("A below C" if med["A"] + spread < med["C"] else "A NOT clearly below C") + ", " + \
                      ("A within the spread of B" if abs(med["A"] - med["B"]) <= spread else f"A {'above' if med['A'] > med['B'] else 'below'} B by {abs(med['A'] / med['B'] - 1) * 100:.1f} %")
            lines.append(f"  {nm:4d} {mode:>4s} | {med['A']:8.4f} {med['B']:8.4f} {med['C']:8.4f} | {spread:7.4f} | {med['A'] / med['B']:6.3f} {med['A'] / med['C']:6.3f} "
                         f"{med['A'] - med['B']:+8.4f} {med['C'] - med['A']:+8.4f}  {verdict}   (|z - C| on four clips: {worst:.1e})")
            print(lines[-1], flush=True)
            for fe in fes:
                fe.close()
            del bufs, mean, inv_std
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
