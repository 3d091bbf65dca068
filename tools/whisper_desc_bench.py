#!/usr/bin/env python3
"""The centred Whisper features from a clip table in device memory (melspec_whisper_compute_ragged_device_desc*) against the host-table
calls, all legs in one run on one box (profiles/whisper_desc.txt).  The clip table (u64 offsets and lengths) is in device memory, as a VAD
or segmenter on the GPU leaves it:
  A   the new call: the tables are read by a planner kernel on the stream
  B   the status quo: the two tables copied to the host (each copy waits for the stream), then the host-table call
  C   the host-table call with the tables already on the host: the floor B starts from
Batches: 1024 ragged clips of 2-20 s at pad_to = 480000; 256 x 30 s.  80 and 128 mels; the default precision mode and F32; normalised
mel-major and split; (F32, F32) and (S16, F16).
Every leg runs on one torch stream (the library's calls are given it).  Every figure is ms per call + synchronise (host clock around REPS
calls and one synchronise, divided by REPS), the legs of a round taken one after the other and the rounds repeated: median [first quartile,
third quartile] over the rounds; ratios are taken per round.  Everything is warmed up first.
  python tools/whisper_desc_bench.py [--rounds 15] [--quick] [--out profiles/whisper_desc.txt]"""
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
from mel_spec_amd.hip import OUT_F16, OUT_F32, PCM_F32, PCM_S16, synth_pcm_device  # noqa: E402

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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whisper_desc.txt"))
    args = ap.parse_args()
    if M.device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("whisper_desc_bench: no gfx950 device visible -- nothing is measured without one")
    dev = torch.device("cuda:0")
    div = 8 if args.quick else 1
    rng = np.random.RandomState(7)
    ragged_lens = (rng.randint(2 * SR, 20 * SR + 1, size=1024 // div)).astype(np.uint64)
    batches = [("1024 ragged 2-20 s, pad_to 480000", ragged_lens), ("256 x 30 s", np.full(256 // div, 30 * SR, np.uint64))]
    pad_to, T = 480000, 3000
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/whisper_desc_bench.py -- {torch.cuda.get_device_name(0)}, source hash {hip_build.source_hash()}, rounds {args.rounds}" + (" (QUICK: not a measurement)" if args.quick else ""))
    say("# ms per call + synchronise: median [Q1, Q3] over the rounds; ratios: median [Q1, Q3] of the per-round ratios")
    say("# A the _desc call (tables in device memory) | B two table copies to the host + the host-table call | C the host-table call, tables on the host")
    side = torch.cuda.Stream()
    st = side.cuda_stream
    for name, lens in batches:
        n = len(lens)
        stride = int(lens.max())
        offs = (np.arange(n, dtype=np.uint64) * np.uint64(stride))
        pcm = torch.zeros(n * stride + 16, dtype=torch.float32, device=dev)
        synth_pcm_device(pcm.data_ptr(), stride, stride, 0, n)
        torch.cuda.synchronize()
        s16 = (pcm * 32767.0).round().clamp(-32768, 32767).to(torch.int16)
        d_offs = torch.from_numpy(offs.astype(np.int64)).to(dev)
        d_lens = torch.from_numpy(lens.astype(np.int64)).to(dev)
        torch.cuda.synchronize()
        for n_mels in (80, 128):
            for mode in ("default", "f32"):
                mel = M.HipMelSpectrogram(400, 160, float(SR), n_mels, device=0)
                if mode != "default":
                    mel.set_precision(mode)
                ne = n * T * n_mels
                out32 = torch.empty(ne + 16, dtype=torch.float32, device=dev)
                out16 = torch.empty(ne + 16, dtype=torch.float16, device=dev)
                gmax = torch.empty(n + 16, dtype=torch.float32, device=dev)
                say(f"\n## {name}, {n_mels} mels, mode {mode}: {n} clips, {n * T} frames -- {M.whisper_kernel_name(mel)}")
                for io in (False, True):
                    x, pd, od, out = (s16, PCM_S16, OUT_F16, out16) if io else (pcm, PCM_F32, OUT_F32, out32)
                    for split in (False, True):
                        if split:
                            def host(o, l):
                                M.whisper_ragged_device_split_io(mel, x.data_ptr(), pd, o, l, out.data_ptr(), od, gmax.data_ptr(), pad_to, None, st)

                            def a_leg():
                                M.whisper_ragged_device_desc_split_io(mel, x.data_ptr(), pd, d_offs.data_ptr(), d_lens.data_ptr(), n, out.data_ptr(), od, gmax.data_ptr(), pad_to, 0, st)
                        else:
                            def host(o, l):
                                M.whisper_ragged_device_io(mel, x.data_ptr(), pd, o, l, out.data_ptr(), od, pad_to, None, True, st)

                            def a_leg():
                                M.whisper_ragged_device_desc_io(mel, x.data_ptr(), pd, d_offs.data_ptr(), d_lens.data_ptr(), n, out.data_ptr(), od, pad_to, 0, True, st)

                        def b_leg():
                            o = d_offs.cpu().numpy().view(np.uint64)          # each copy waits for the stream
                            l = d_lens.cpu().numpy().view(np.uint64)
                            host(o, l)

                        legs = {"A": a_leg, "B": b_leg, "C": lambda: host(offs, lens)}
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
                        say(f"  {'(S16, F16)' if io else '(F32, F32)'} {'split     ' if split else 'normalised'}  A {fmt(times['A'])}  B {fmt(times['B'])}  C {fmt(times['C'])} ms"
                            f"   A/B {ratio(times['A'], times['B'])}   A/C {ratio(times['A'], times['C'])}")
                mel.close()
                del out32, out16, gmax
        del pcm, s16
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
