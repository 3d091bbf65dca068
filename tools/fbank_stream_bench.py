#!/usr/bin/env python3
"""Kaldi fbank stream bank: melspec_fbank_stream_push_device against the nearest existing things, in one process on one GPU
(profiles/fbank_stream.txt).  Recorded, not gated.

Shape: 1024 live streams, default FbankConfig (16 kHz, 25 ms / 10 ms, 80 bins), chunks of 10 ms, 100 ms and 1 s (160 / 1600 / 16000
samples) already in device memory, noise.  Per chunk size, three variants, each on objects of its own:
  F  melspec_fbank_stream_push_device, chunks at melspec_fbank_stream_input_ptr: frames + column sums + carry
  W  melspec_stream_push_device of the Whisper bank (400 / 160 / 80) at the same sizes: the nearest existing streaming call
  R  melspec_fbank_compute_ragged_device on the history ++ chunk batch (frame_len - shift = 240 samples of history per stream, apply_cmn
     off) + melspec_fbank_synchronize: what a caller does today, WITHOUT the copies that keep its history up to date
Every call returns after its work has completed (F, W by contract, R by the synchronise), so a call is timed on the host clock around
it.  --rounds rounds of --calls calls per variant after --warmup calls each (which also take every stream past its first frame); a round
times every variant once, even rounds in the order F W R, odd rounds reversed.  Per variant: the median of the rounds' mean call time and
their spread (max - min).

Measured (MI355X, 1024 streams; ms per push, median of 7 rounds x 30 pushes, spreads 0.0003 - 0.0075; profiles/fbank_stream.txt):
  chunk (samples)   rows / push      F ms      W ms      R ms    F / W   F / R
        160 (10 ms)       1024    0.0514    0.0352    0.0307     1.46    1.67
       1600 (100 ms)     10240    0.0584    0.0361    0.0360     1.62    1.62
      16000 (1 s)       102400    0.1295    0.0589    0.0804     2.20    1.61
The bank is the slowest of the three at every size: 1.5 - 2.2 x the Whisper bank's push (which reuses its previous plan in steady state;
this bank plans and uploads every push) and 1.6 - 1.7 x the bare ragged call -- which leaves out what its caller must still do (keep the
history, assemble the batch, the column sums).  A push is five launches (entry table, plan, frames, column sums, carry) against two.

  python tools/fbank_stream_bench.py [--out profiles/fbank_stream.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fbank_stream.txt"))
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
    n, nm, shift, frame_len = args.streams, 80, 160, 400
    hist = frame_len - shift
    rng = np.random.default_rng(4321)
    ids = np.arange(n, dtype=np.uint32)
    fb = M.Fbank(M.FbankConfig())
    fb0 = M.Fbank(M.FbankConfig(apply_cmn=False))
    mel = M.HipMelSpectrogram(400, shift, 16000.0, nm)
    lines = [f"# tools/fbank_stream_bench.py -- library source hash {hip_build.source_hash()}",
             f"# {n} streams, 16 kHz, 25 ms / 10 ms, {nm} bins; {args.rounds} rounds x {args.calls} calls per variant, order F W R and its reverse in turn, after "
             f"{args.warmup} warm-up calls each; host clock around calls that return after their work has completed",
             "# F fbank stream push_device (frames + column sums + carry)   W Whisper bank push_device   R fbank compute_ragged_device on history ++ chunk + synchronize",
             f"# {'chunk':>7s} {'rows/push':>10s} | {'F ms':>8s} {'spread':>7s} | {'W ms':>8s} {'spread':>7s} | {'R ms':>8s} {'spread':>7s} | {'F / W':>6s} {'F / R':>6s}"]
    for chunk in (160, 1600, 16000):
        lens = np.full(n, chunk, np.uint32)
        rows = chunk // shift
        out = M.DeviceBuffer(n * rows * nm * 4)
        fbank_bank = M.FbankStreamBank(fb, n, chunk)
        whisper_bank = M.StreamBank(mel, n, chunk)
        pcm = (rng.standard_normal((n, hist + chunk)) * 0.1).astype(np.float32)
        for bank in (fbank_bank, whisper_bank):          # the chunks stay where a push leaves them: written once
            p0 = bank.input_ptr(0)
            step = bank.input_ptr(1) - p0 if n > 1 else 0
            for s in range(n):
                c = np.ascontiguousarray(pcm[s, hist:])
                assert lib.melspec_memcpy_h2d(C.c_void_p(p0 + s * step), c.ctypes.data_as(C.c_void_p), c.nbytes) == 0
        d_pcm = M.DeviceBuffer(pcm.nbytes)
        d_pcm.upload(pcm)
        offs = np.arange(n, dtype=np.uint64) * (hist + chunk)
        clip_lens = np.full(n, hist + chunk, np.uint64)
        assert fb0.num_frames(hist + chunk) == rows

        def run_f():
            assert (fbank_bank.push_device(ids, lens, out.ptr) <= rows).all()

        def run_w():
            whisper_bank.push_device(ids, lens, out.ptr)

        def run_r():
            fb0.compute_ragged_device(d_pcm.ptr, offs, clip_lens, out.ptr)
            fb0.synchronize()

        variants = [("F", run_f), ("W", run_w), ("R", run_r)]
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
        lines.append(f"  {chunk:7d} {n * rows:10d} | {med['F']:8.4f} {spread['F']:7.4f} | {med['W']:8.4f} {spread['W']:7.4f} | {med['R']:8.4f} {spread['R']:7.4f} | "
                     f"{med['F'] / med['W']:6.2f} {med['F'] / med['R']:6.2f}")
        fbank_bank.close(); whisper_bank.close(); out.free(); d_pcm.free()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)
    fb.close(); fb0.close(); mel.close()


if __name__ == "__main__":
    main()
