#!/usr/bin/env python3
"""The resampler (melspec_resample_*) against the status quo in torch, all legs in one run on one box (profiles/resample.txt).  The
batch is resident in HBM: 1024 x 10 s clips at 48000, 44100 and 8000 Hz -> 16000 Hz, and 1024 ragged clips of 2-20 s at 48000 Hz.
  A    the new call, (S16) in: int16 PCM -> f32 PCM at 16 kHz, one launch
  A32  the new call, (F32) in
  B    the status quo on the same GPU: int16 -> f32 cast, zero pad, conv1d(stride = orig) with the dense [new][K] kernel of the
       definition in f32 (what torchaudio.functional.resample does), reshape and truncate.  The ragged batch: padded to the longest clip.
Every leg runs on one torch stream (the library's calls are given it).  Every figure is ms per call + synchronise (host clock around REPS
calls and one synchronise, divided by REPS), the legs of a round taken one after the other and the rounds repeated: median [first quartile,
third quartile] over the rounds; ratios are taken per round.  Everything is warmed up first.  frac: A's own bytes (samples read + outputs
written) / time / 8 TB/s.
  python tools/resample_bench.py [--rounds 15] [--quick] [--out profiles/resample.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch          # before libmelspec_hip.so is loaded

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mel_spec_amd as M                      # noqa: E402
from mel_spec_amd import build as hip_build   # noqa: E402
from mel_spec_amd import resample             # noqa: E402

HBM_PEAK = 8.0e12


def quartiles(v):
    q1, q2, q3 = np.percentile(np.asarray(v), [25, 50, 75])
    return q2, q1, q3


def fmt(v):
    q2, q1, q3 = quartiles(v)
    return f"{q2:8.4f} [{q1:8.4f}, {q3:8.4f}]"


def ratio(a, b):
    """median of the per-round ratios and their quartiles"""
    return quartiles(np.asarray(a) / np.asarray(b))


def verdict(name, a, b):
    q2, q1, q3 = ratio(a, b)
    text = f"{name} {q2:6.3f} [{q1:6.3f}, {q3:6.3f}]"
    if q3 >= 1.0:
        text += f"  {name.split('/')[0].strip()} IS NOT BELOW {name.split('/')[1].strip()} BEYOND THE SPREAD"
    return text


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="an eighth of the clips (a rehearsal, not a measurement)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample.txt"))
    args = ap.parse_args()
    if M.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("resample_bench: no gfx950 device visible -- nothing is measured without one")
    dev = torch.device("cuda:0")
    n_clips = 1024 // (8 if args.quick else 1)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/resample_bench.py -- {torch.cuda.get_device_name(0)}, source hash {hip_build.source_hash()}, rounds {args.rounds}" + (" (QUICK: not a measurement)" if args.quick else ""))
    say("# ms per call + synchronise: median [Q1, Q3] over the rounds; ratios: median [Q1, Q3] of the per-round ratios")
    say("# A the new call, int16 in | A32 the new call, f32 in | B torch: int16 -> f32 cast, zero pad, conv1d(stride = orig) with the dense f32 kernel, reshape, truncate")
    side = torch.cuda.Stream()
    st = side.cuda_stream
    gen = torch.Generator(device=dev).manual_seed(4321)
    rng = np.random.RandomState(7)
    rows = [(48000, None), (44100, None), (8000, None), (48000, rng.randint(2 * 48000, 20 * 48000 + 1, size=n_clips).astype(np.uint64))]
    for rate_in, lens in rows:
        rate_out = 16000
        orig, new, width, taps = resample.geometry(rate_in, rate_out)
        K = 2 * width + orig
        rs = M.Resampler(rate_in, rate_out, device=0)
        n = 10 * rate_in if lens is None else int(lens.max())
        n_out = rs.out_len(n)
        s16 = torch.randint(-9830, 9831, (n_clips, n), generator=gen, device=dev, dtype=torch.int32).to(torch.int16)
        f32 = s16.to(torch.float32) / 32768.0
        out = torch.empty((n_clips, n_out), dtype=torch.float32, device=dev)
        h = torch.from_numpy(resample.taps(rate_in, rate_out).astype(np.float32)).to(dev).reshape(new, 1, K)
        if lens is None:
            name = f"{n_clips} x 10 s at {rate_in} Hz"
            own = n_clips * (n * 2 + n_out * 4)
            own32 = n_clips * (n * 4 + n_out * 4)

            def a_leg():
                rs.compute_uniform_device(s16.data_ptr(), "s16", n, n, n_clips, out.data_ptr(), n_out, st)

            def a32_leg():
                rs.compute_uniform_device(f32.data_ptr(), "f32", n, n, n_clips, out.data_ptr(), n_out, st)
        else:
            name = f"{n_clips} ragged clips of 2-20 s at {rate_in} Hz (B: padded to the longest, {n / rate_in:.1f} s)"
            offs = np.arange(n_clips, dtype=np.uint64) * np.uint64(n)
            oo = np.arange(n_clips, dtype=np.uint64) * np.uint64(n_out)
            total_in, total_out = int(lens.sum()), int(sum(rs.out_len(int(v)) for v in lens))
            own = total_in * 2 + total_out * 4
            own32 = total_in * 4 + total_out * 4

            def a_leg():
                rs.compute_ragged_device(s16.data_ptr(), "s16", offs, lens, out.data_ptr(), oo, st)

            def a32_leg():
                rs.compute_ragged_device(f32.data_ptr(), "f32", offs, lens, out.data_ptr(), oo, st)

        def b_leg():
            x = s16.to(torch.float32) / 32768.0
            x = torch.nn.functional.pad(x, (width, width + orig))
            y = torch.nn.functional.conv1d(x[:, None, :], h, stride=orig)          # [clips][new][blocks]
            return y.transpose(1, 2).reshape(n_clips, -1)[:, :n_out].contiguous()

        legs = {"A": a_leg, "A32": a32_leg, "B": b_leg}
        reps = 3
        times = {k: [] for k in legs}
        with torch.cuda.stream(side):
            for f in legs.values():          # warm-up: code objects, tables, the allocator's blocks, the convolution's choice of algorithm
                for _ in range(3):
                    f()
            side.synchronize()
            # the two routes agree (B sums in f32): a glance, the tests hold the contract
            a_leg()
            side.synchronize()
            head = rs.out_len(2 * rate_in) - 64          # inside every clip of the ragged batch, clear of its end
            d = float((out[:8, :head] - b_leg()[:8, :head]).abs().max())
            for _ in range(args.rounds):
                for k, f in legs.items():
                    t0 = time.perf_counter()
                    for _ in range(reps):
                        f()
                    side.synchronize()
                    times[k].append((time.perf_counter() - t0) * 1e3 / reps)
        a_ms, a32_ms = quartiles(times["A"])[0], quartiles(times["A32"])[0]
        say(f"\n## {name}: {orig} : {new}, {taps} inside taps -- {rs.kernel_name}; max |A - B| on 8 x 2 s = {d:.2e}")
        say(f"  A   {fmt(times['A'])} ms   frac {own / (a_ms * 1e-3) / HBM_PEAK:5.3f} of 8 TB/s on {own / 1e9:.2f} GB")
        say(f"  A32 {fmt(times['A32'])} ms   frac {own32 / (a32_ms * 1e-3) / HBM_PEAK:5.3f} of 8 TB/s on {own32 / 1e9:.2f} GB")
        say(f"  B   {fmt(times['B'])} ms")
        say(f"  {verdict('A / B', times['A'], times['B'])}")
        say(f"  {verdict('A32 / B', times['A32'], times['B'])}")
        rs.close()
        del s16, f32, out, h
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
