#!/usr/bin/env python3
"""NeMo / Parakeet stream bank: melspec_blm_stream_push_device against the nearest existing things, in one process on one GPU
(profiles/blm_stream.txt).  Recorded, not gated.

Shape: 1024 live streams, default BatchLogMelConfig (16 kHz, n_fft 512 / win 400 / hop 160, 80 mels, centred), chunks of 10 ms, 100 ms
and 1 s (160 / 1600 / 16000 samples) already in device memory, noise; in the default f64 mode and in MELSPEC_PRECISION_F32.  Per chunk
size, three variants, each on objects of its own:
  N  melspec_blm_stream_push_device, chunks at melspec_blm_stream_input_ptr: columns + running statistics + carry
  K  melspec_fbank_stream_push_device of the Kaldi bank (25 ms / 10 ms, 80 bins) at the same sizes: the nearest existing streaming call
     (f64 whatever the mode)
  R  melspec_blm_compute_ragged_device on the history ++ chunk batch -- a center = 0 context, n_fft - hop = 352 samples of history per
     stream, which yields exactly the chunk's frames -- + melspec_blm_synchronize: what a caller does today, WITHOUT the copies that
     keep its history up to date and without any statistics
Every call returns after its work has completed (N, K by contract, R by the synchronise), so a call is timed on the host clock around
it.  --rounds rounds of --calls calls per variant after --warmup calls each (which also take every stream past its first frame); a round
times every variant once, even rounds in the order N K R, odd rounds reversed.  Per variant: the median of the rounds' mean call time and
their spread (max - min).

  python tools/blm_stream_bench.py [--out profiles/blm_stream.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blm_stream.txt"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()

    import numpy as np
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd._lib import lib as load
    lib = load()
    assert M.device_count() >= 1, "no GPU: nothing to measure"
    n, nm, hop, n_fft = args.streams, 80, 160, 512
    hist = n_fft - hop
    rng = np.random.default_rng(4321)
    ids = np.arange(n, dtype=np.uint32)
    lines = [f"# tools/blm_stream_bench.py -- library source hash {hip_build.source_hash()}",
             f"# {n} streams, 16 kHz, n_fft 512 / win 400 / hop 160, {nm} mels; {args.rounds} rounds x {args.calls} calls per variant, order N K R and its reverse in turn, after "
             f"{args.warmup} warm-up calls each; host clock around calls that return after their work has completed",
             "# N blm stream push_device (columns + running statistics + carry)   K Kaldi fbank stream push_device   R blm compute_ragged_device (center = 0) on history ++ chunk + synchronize",
             f"# {'mode':>5s} {'chunk':>7s} {'cols/push':>10s} | {'N ms':>8s} {'spread':>7s} | {'K ms':>8s} {'spread':>7s} | {'R ms':>8s} {'spread':>7s} | {'N / K':>6s} {'N / R':>6s}"]
    fb = M.Fbank(M.FbankConfig())
    for mode in ("f64", "f32"):
        fe = M.BatchLogMelSpectrogram(M.BatchLogMelConfig())
        fe0 = M.BatchLogMelSpectrogram(M.BatchLogMelConfig(center=False))
        fe.set_precision(mode); fe0.set_precision(mode)
        assert fe.precision == mode and fe0.precision == mode
        for chunk in (160, 1600, 16000):
            lens = np.full(n, chunk, np.uint32)
            cols = chunk // hop
            out = M.DeviceBuffer(n * cols * nm * 4)
            blm_bank = M.BlmStreamBank(fe, n, chunk)
            kaldi_bank = M.FbankStreamBank(fb, n, chunk)
            pcm = (rng.standard_normal((n, hist + chunk)) * 0.1).astype(np.float32)
            for bank in (blm_bank, kaldi_bank):              # the chunks stay where a push leaves them: written once
                p0 = bank.input_ptr(0)
                step = bank.input_ptr(1) - p0 if n > 1 else 0
                for s in range(n):
                    c = np.ascontiguousarray(pcm[s, hist:])
                    assert lib.melspec_memcpy_h2d(C.c_void_p(p0 + s * step), c.ctypes.data_as(C.c_void_p), c.nbytes) == 0
            d_pcm = M.DeviceBuffer(pcm.nbytes)
            d_pcm.upload(pcm)
            offs = np.arange(n, dtype=np.uint64) * (hist + chunk)
            clip_lens = np.full(n, hist + chunk, np.uint64)
            assert fe0.num_frames(hist + chunk) == cols

            def run_n():
                assert (blm_bank.push_device(ids, lens, out.ptr) <= cols).all()

            def run_k():
                kaldi_bank.push_device(ids, lens, out.ptr)

            def run_r():
                fe0.compute_ragged_device(d_pcm.ptr, offs, clip_lens, out.ptr)
                fe0.synchronize()

            variants = [("N", run_n), ("K", run_k), ("R", run_r)]
            for _ in range(args.warmup):
                for _, fn in variants:
                    fn()
            ms = {k: [] for k, _ in variants}
            for r in range(args.rounds):
                for label, fn in (variants if r % 2 == 0 else variants[::-1]):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    ms[label].append((time.perf_counter() - t0) * 1e3 / args.calls)
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            lines.append(f"  {mode:>5s} {chunk:7d} {n * cols:10d} | {med['N']:8.4f} {spread['N']:7.4f} | {med['K']:8.4f} {spread['K']:7.4f} | {med['R']:8.4f} {spread['R']:7.4f} | "
                         f"{med['N'] / med['K']:6.2f} {med['N'] / med['R']:6.2f}")
            blm_bank.close(); kaldi_bank.close(); out.free(); d_pcm.free()
        fe.close(); fe0.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)
    fb.close()


if __name__ == "__main__":
    main()
