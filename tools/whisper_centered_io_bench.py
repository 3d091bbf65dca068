#!/usr/bin/env python3
"""The centred Whisper features with int16 PCM in / f16 out (melspec_whisper_*_io) against the f32 calls, all legs in one run on one box
(profiles/whisper_centered_io.txt).  The audio is int16 and the consumer takes f16, mel-major:
  A   the f32 normalised call on the batch already converted to f32 (the conversion is not timed): the floor the status quo starts from
  B   the status quo: torch int16 -> f32 conversion (to(float32) * 2^-15), A, torch cast of the features to f16
  D   the new normalised call (S16, F16)
  S   the f32 split call (raw rows + clip maxima)        Ds  the new split call (S16, F16)
Batches: 256 x 30 s; 1024 ragged clips of 2-20 s at pad_to = 480000.  80 and 128 mels; the default precision mode and F32.
Every leg runs on one torch stream (the library's calls are given it), so B's three steps are ordered like a user's.  Every figure is ms
per call + synchronise (host clock around REPS calls and one synchronise, divided by REPS), the legs of a round taken one after the other
and the rounds repeated: median [first quartile, third quartile] over the rounds; ratios are taken per round.  Everything is warmed up first.
  python tools/whisper_centered_io_bench.py [--rounds 15] [--quick]"""
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
from mel_spec_amd.hip import OUT_F16, PCM_S16, synth_pcm_device  # noqa: E402

SR = 16000


def quartiles(v):
    q1, q2, q3 = np.percentile(np.asarray(v), [25, 50, 75])
    return q2, q1, q3


def fmt(v):
    q2, q1, q3 = quartiles(v)
    return f"{q2:8.4f} [{q1:8.4f}, {q3:8.4f}]"


def ratio(a, b):
    """median of the per-round ratios and their quartiles"""
    q2, q1, q3 = quartiles(np.asarray(a) / np.asarray(b))
    return f"{q2:6.3f} [{q1:6.3f}, {q3:6.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--quick", action="store_true", help="an eighth of the clips (a rehearsal, not a measurement)")
    args = ap.parse_args()
    if M.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("whisper_centered_io_bench: no gfx950 device visible -- nothing is measured without one")
    dev = torch.device("cuda:0")
    div = 8 if args.quick else 1
    rng = np.random.RandomState(7)
    ragged_lens = (rng.randint(2 * SR, 20 * SR + 1, size=1024 // div)).astype(np.uint64)
    batches = [("256 x 30 s", np.full(256 // div, 30 * SR, np.uint64), 480000),
               ("1024 ragged 2-20 s, pad_to 480000", ragged_lens, 480000)]
    print(f"# tools/whisper_centered_io_bench.py -- {torch.cuda.get_device_name(0)}, source hash {hip_build.source_hash()}, rounds {args.rounds}" + (" (QUICK: not a measurement)" if args.quick else ""))
    print("# ms per call + synchronise: median [Q1, Q3] over the rounds; ratios: median [Q1, Q3] of the per-round ratios")
    print("# A f32 call (input already f32) | B torch int16->f32, A, torch f32->f16 | D (S16, F16) call | S f32 split | Ds (S16, F16) split; mel-major")
    side = torch.cuda.Stream()
    st = side.cuda_stream
    for name, lens, pad_to in batches:
        n = len(lens)
        uniform = bool(np.all(lens == lens[0]))
        stride = int(lens.max())
        offs = (np.arange(n, dtype=np.uint64) * np.uint64(stride))
        pcm = torch.zeros(n * stride + 16, dtype=torch.float32, device=dev)
        synth_pcm_device(pcm.data_ptr(), stride, stride, 0, n)
        torch.cuda.synchronize()
        s16 = (pcm * 32767.0).round().clamp(-32768, 32767).to(torch.int16)          # the audio as it arrives
        pcm = s16.to(torch.float32) * (2.0 ** -15)                                   # A's input: the same samples
        torch.cuda.synchronize()
        for n_mels in (80, 128):
            for mode in ("default", "f32"):
                mel = M.HipMelSpectrogram(400, 160, float(SR), n_mels, device=0)
                if mode != "default":
                    mel.set_precision(mode)
                Ts = [M.whisper_num_frames(mel, int(v), pad_to) for v in lens]
                total = int(sum(Ts))
                ne = total * n_mels
                out32 = torch.empty(ne + 16, dtype=torch.float32, device=dev)
                out16 = torch.empty(ne + 16, dtype=torch.float16, device=dev)
                gmax = torch.empty(n + 16, dtype=torch.float32, device=dev)
                if uniform:
                    def a_leg(x):
                        M.whisper_uniform_device(mel, x.data_ptr(), stride, stride, n, out32.data_ptr(), pad_to, True, st)
                    legs = {"D": lambda: M.whisper_uniform_device_io(mel, s16.data_ptr(), PCM_S16, stride, stride, n, out16.data_ptr(), OUT_F16, pad_to, True, st),
                            "S": lambda: M.whisper_uniform_device_split(mel, pcm.data_ptr(), stride, stride, n, out32.data_ptr(), gmax.data_ptr(), pad_to, st),
                            "Ds": lambda: M.whisper_uniform_device_split_io(mel, s16.data_ptr(), PCM_S16, stride, stride, n, out16.data_ptr(), OUT_F16, gmax.data_ptr(), pad_to, st)}
                else:
                    def a_leg(x):
                        M.whisper_ragged_device(mel, x.data_ptr(), offs, lens, out32.data_ptr(), pad_to, None, True, st)
                    legs = {"D": lambda: M.whisper_ragged_device_io(mel, s16.data_ptr(), PCM_S16, offs, lens, out16.data_ptr(), OUT_F16, pad_to, None, True, st),
                            "S": lambda: M.whisper_ragged_device_split(mel, pcm.data_ptr(), offs, lens, out32.data_ptr(), gmax.data_ptr(), pad_to, None, st),
                            "Ds": lambda: M.whisper_ragged_device_split_io(mel, s16.data_ptr(), PCM_S16, offs, lens, out16.data_ptr(), OUT_F16, gmax.data_ptr(), pad_to, None, st)}

                def b_leg():
                    x = s16.to(torch.float32).mul_(2.0 ** -15)
                    a_leg(x)
                    return out32[:ne].to(torch.float16)

                legs = {"A": lambda: a_leg(pcm), "B": b_leg, **legs}
                reps = 5
                times = {k: [] for k in legs}
                with torch.cuda.stream(side):
                    for f in legs.values():          # warm-up: code objects, scratch, plans, the allocator's blocks
                        for _ in range(3):
                            f()
                    side.synchronize()
                    for _ in range(args.rounds):
                        for k, f in legs.items():
                            t0 = time.perf_counter()
                            for _ in range(reps):
                                f()
                            side.synchronize()
                            times[k].append((time.perf_counter() - t0) * 1e3 / reps)
                print(f"\n## {name}, {n_mels} mels, mode {mode}: {n} clips, {total} frames -- {M.whisper_kernel_name(mel)}")
                for k in times:
                    print(f"  {k:3s} {fmt(times[k])} ms   {total / quartiles(times[k])[0] / 1e6:7.2f} G frames/s")
                print(f"  D/B {ratio(times['D'], times['B'])}   D/A {ratio(times['D'], times['A'])}   B/A {ratio(times['B'], times['A'])}   Ds/S {ratio(times['Ds'], times['S'])}   D/Ds {ratio(times['D'], times['Ds'])}")
                mel.close()
                del out32, out16, gmax
        del pcm, s16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
