#!/usr/bin/env python3
"""NeMo / Parakeet frontend, ragged batches whose clip table is produced on the GPU: melspec_blm_compute_ragged_device_desc (the plan built
by a kernel from device tables) against what a caller had to do before it existed, and against the host-table call with the tables
already on the host, in one process on one GPU (profiles/blm_desc.txt).

Shape: 1024 clips of noise, lengths drawn (seeded) uniformly from 2 s to 20 s, at 80 and 128 mels, default (f64) and
MELSPEC_PRECISION_F32 arithmetic, normalize_per_feature off and on.  Variants:
  A  melspec_blm_compute_ragged_device_desc, offsets and lengths resident on the device, exact bounds
  B  what A replaces: the two tables copied to the host (one synchronous copy each: the copy and its synchronise), then
     melspec_blm_compute_ragged_device
  C  melspec_blm_compute_ragged_device with the tables already on the host -- its kernels are the parent commit's
Every timed call is one call followed by a synchronise of its stream, timed with the host clock.  After a warm-up of every variant a
round times each variant once, even rounds in the order A B C, odd rounds in reverse; per variant the median of the rounds and their
spread (max - min).

  python tools/blm_desc_bench.py [--out profiles/blm_desc.txt]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blm_desc.txt"))
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
    # the device-resident tables (u64 as int64 bit patterns) and the pageable host arrays variant B copies them into
    d_offs, d_lens = torch.from_numpy(offs.view(np.int64)).to(dev), torch.from_numpy(lens.view(np.int64)).to(dev)
    h_offs, h_lens = np.empty(args.clips, np.uint64), np.empty(args.clips, np.uint64)
    d_rej = torch.zeros((4,), device=dev, dtype=torch.int32)

    lines = [f"# tools/blm_desc_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {args.clips} clips of noise, 2 s .. 20 s (seeded), {total / 16000:.0f} s in all; {args.rounds} rounds, a round = one call of each variant ending in a synchronise "
             f"(host clock), order A B C and its reverse in turn, after {args.warmup} warm-up calls each; ms per call, median of the rounds",
             "# A the _desc call, tables on the device; B two tables copied to the host (with their synchronise) + the host-table ragged call; C the host-table ragged call, tables on the host",
             f"# {'mels':>4s} {'mode':>4s} {'norm':>4s} | {'A':>8s} {'B':>8s} {'C':>8s} | {'spread':>7s} | {'A / B':>6s} {'A / C':>6s} {'B - A':>8s} {'A - C':>8s}  verdict"]
    for nm in (80, 128):
        for mode in ("f64", "f32"):
            for norm in (False, True):
                fe = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(n_mels=nm, normalize_per_feature=norm), device=0)
                fe.set_precision(mode)
                assert fe.precision == mode
                cols = int(sum(fe.padded_frames(int(n)) for n in lens))
                longest = int(lens.max())
                bufs = {k: torch.empty((cols * nm,), device=dev, dtype=torch.float32) for k in "ABC"}

                def timed(fn):
                    def run():
                        t0 = time.perf_counter()
                        fn()
                        fe.synchronize(stream)
                        return (time.perf_counter() - t0) * 1e3
                    return run

                def variant_b():
                    h_offs[:] = d_offs.cpu().numpy().view(np.uint64)          # a synchronous device-to-host copy each
                    h_lens[:] = d_lens.cpu().numpy().view(np.uint64)
                    fe.compute_ragged_device(pcm.data_ptr(), h_offs, h_lens, bufs["B"].data_ptr(), None, stream)
                variants = [
                    ("A", timed(lambda: M.blm_compute_ragged_device_desc(fe, pcm.data_ptr(), d_offs.data_ptr(), d_lens.data_ptr(), args.clips, bufs["A"].data_ptr(), 0,
                                                                         cols, longest, d_rej.data_ptr(), stream))),
                    ("B", timed(variant_b)),
                    ("C", timed(lambda: fe.compute_ragged_device(pcm.data_ptr(), offs, lens, bufs["C"].data_ptr(), None, stream))),
                ]
                # before anything is timed: the three outputs are the same bits, nobody was rejected
                for _, fn in variants:
                    fn()
                torch.cuda.synchronize()
                assert torch.equal(bufs["A"].view(torch.int32), bufs["C"].view(torch.int32)), "A's output is not the host-table call's bits"
                assert torch.equal(bufs["B"].view(torch.int32), bufs["C"].view(torch.int32))
                assert int(d_rej[0]) == 0
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
                verdict = ("A below B" if med["A"] + iqr < med["B"] else "A NOT clearly below B") + ", " + \
                          ("A within the quartiles of C" if abs(med["A"] - med["C"]) <= iqr else f"A {'above' if med['A'] > med['C'] else 'below'} C by {abs(med['A'] / med['C'] - 1) * 100:.1f} %")
                lines.append(f"  {nm:4d} {mode:>4s} {'on' if norm else 'off':>4s} | {med['A']:8.4f} {med['B']:8.4f} {med['C']:8.4f} | {spread:7.4f} | {med['A'] / med['B']:6.3f} {med['A'] / med['C']:6.3f} "
                             f"{med['B'] - med['A']:+8.4f} {med['A'] - med['C']:+8.4f}  {verdict}   (widest interquartile range {iqr:.4f})")
                print(lines[-1], flush=True)
                fe.close()
                del bufs
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
