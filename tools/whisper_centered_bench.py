#!/usr/bin/env python3
"""The centred Whisper features (melspec_whisper_*) against their neighbours, all legs in one run on one box (profiles/whisper_centered.txt):
  A   the normalised call, mel-major            A'  the normalised call, frame-major          S  the split call (raw rows + clip maxima)
  B   the existing melspec_compute_*_device on the same PCM: the per-frame variant, the nearest existing kernel and the floor for S
  C   the openai-whisper recipe in torch on the same GPU, f32 (torch.stft(center=True), filters @ |X|^2, log10, clip-wide clamp): what a
      user of a Whisper checkpoint runs today.  C gets its batch already padded to pad_to as one [clips, samples] tensor.
Batches: 1024 x 10 s at pad_to = 0; 256 x 30 s; 1024 ragged clips of 2-20 s at pad_to = 480000.  80 and 128 mels, F64 and F32.
Every figure is ms per call + synchronise (host clock around REPS calls and one synchronise, divided by REPS), the legs of a round taken one
after the other and the rounds repeated: median [first quartile, third quartile] over the rounds.  Everything is warmed up first.
  python tools/whisper_centered_bench.py [--rounds 15] [--quick]"""
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
from mel_spec_amd.hip import synth_pcm_device  # noqa: E402
from oracle import oracle as O                # noqa: E402

SR = 16000


def torch_recipe(x, filters, window):
    stft = torch.stft(x, 400, 160, window=window, center=True, pad_mode="reflect", return_complex=True)
    mag = stft[..., :-1].abs() ** 2
    log = torch.clamp(filters @ mag, min=1e-10).log10()
    log = torch.maximum(log, log.amax(dim=(-2, -1), keepdim=True) - 8.0)
    return (log + 4.0) / 4.0


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
        raise SystemExit("whisper_centered_bench: no gfx950 device visible -- nothing is measured without one")
    dev = torch.device("cuda:0")
    div = 8 if args.quick else 1
    rng = np.random.RandomState(7)
    ragged_lens = (rng.randint(2 * SR, 20 * SR + 1, size=1024 // div)).astype(np.uint64)
    batches = [("1024 x 10 s, pad_to 0", np.full(1024 // div, 10 * SR, np.uint64), 0),
               ("256 x 30 s", np.full(256 // div, 30 * SR, np.uint64), 480000),
               ("1024 ragged 2-20 s, pad_to 480000", ragged_lens, 480000)]
    print(f"# tools/whisper_centered_bench.py -- {torch.cuda.get_device_name(0)}, source hash {hip_build.source_hash()}, rounds {args.rounds}" + (" (QUICK: not a measurement)" if args.quick else ""))
    print("# ms per call + synchronise: median [Q1, Q3] over the rounds; ratios: median [Q1, Q3] of the per-round ratios")
    window = torch.hann_window(400, periodic=True, device=dev)
    for name, lens, pad_to in batches:
        n = len(lens)
        uniform = bool(np.all(lens == lens[0]))
        stride = int(lens.max())
        offs = (np.arange(n, dtype=np.uint64) * np.uint64(stride))
        pcm = torch.zeros(n * stride + 16, dtype=torch.float32, device=dev)
        synth_pcm_device(pcm.data_ptr(), stride, stride, 0, n)
        torch.cuda.synchronize()
        # C's input: the clips cut to their lengths and zero-extended to pad_to (pad_to 0: the clips themselves)
        P = pad_to if pad_to else stride
        xc = torch.zeros(n, P, dtype=torch.float32, device=dev)
        view = pcm[:n * stride].view(n, stride)
        w = min(P, stride)
        xc[:, :w] = view[:, :w]
        if not uniform:
            keep = torch.arange(P, device=dev)[None, :] < torch.from_numpy(lens.astype(np.int64)).to(dev)[:, None]
            xc = xc * keep
        for n_mels in (80, 128):
            filters = torch.from_numpy(O.mel_filterbank(float(SR), 400, n_mels).astype(np.float32)).to(dev)
            mel = M.HipMelSpectrogram(400, 160, float(SR), n_mels, device=0)
            T = M.whisper_num_frames(mel, int(lens[0]), pad_to)
            Ts = [M.whisper_num_frames(mel, int(v), pad_to) for v in lens]
            total = int(sum(Ts))
            out = torch.empty(total * n_mels + 16, dtype=torch.float32, device=dev)
            gmax = torch.empty(n + 16, dtype=torch.float32, device=dev)
            fB = [mel.num_frames(int(v)) for v in lens]
            outB = torch.empty(int(sum(fB)) * n_mels + 16, dtype=torch.float32, device=dev)
            silent = sum(max(0, t - max(2, -(-(min(int(v), pad_to or int(v)) + 200) // 160))) for t, v in zip(Ts, lens)) if pad_to else 0
            print(f"\n## {name}, {n_mels} mels: {n} clips, {total} frames ({silent} silent), T {T if uniform or pad_to else 'ragged'}")
            legs = {}
            if uniform:
                legs["A"] = lambda: M.whisper_uniform_device(mel, pcm.data_ptr(), stride, stride, n, out.data_ptr(), pad_to, True)
                legs["A'"] = lambda: M.whisper_uniform_device(mel, pcm.data_ptr(), stride, stride, n, out.data_ptr(), pad_to, False)
                legs["S"] = lambda: M.whisper_uniform_device_split(mel, pcm.data_ptr(), stride, stride, n, out.data_ptr(), gmax.data_ptr(), pad_to)
                legs["B"] = lambda: mel.compute_uniform_device(pcm.data_ptr(), stride, stride, n, outB.data_ptr())
            else:
                legs["A"] = lambda: M.whisper_ragged_device(mel, pcm.data_ptr(), offs, lens, out.data_ptr(), pad_to, None, True)
                legs["A'"] = lambda: M.whisper_ragged_device(mel, pcm.data_ptr(), offs, lens, out.data_ptr(), pad_to, None, False)
                legs["S"] = lambda: M.whisper_ragged_device_split(mel, pcm.data_ptr(), offs, lens, out.data_ptr(), gmax.data_ptr(), pad_to)
                legs["B"] = lambda: mel.compute_ragged_device(pcm.data_ptr(), offs, lens, outB.data_ptr())
            c_leg = lambda: torch_recipe(xc, filters, window)
            for mode in ("f64", "f32"):
                mel.set_precision(mode)
                reps = 5
                for f in legs.values():          # warm-up: code objects, scratch, plans
                    for _ in range(3):
                        f()
                for _ in range(2):
                    c_leg()
                mel.synchronize(); torch.cuda.synchronize()
                times = {k: [] for k in list(legs) + ["C"]}
                for _ in range(args.rounds):
                    for k, f in legs.items():
                        t0 = time.perf_counter()
                        for _ in range(reps):
                            f()
                        mel.synchronize()
                        times[k].append((time.perf_counter() - t0) * 1e3 / reps)
                    t0 = time.perf_counter()
                    for _ in range(2):
                        c_leg()
                    torch.cuda.synchronize()
                    times["C"].append((time.perf_counter() - t0) * 1e3 / 2)
                print(f"# mode {mode}: {M.whisper_kernel_name(mel)}")
                for k in times:
                    print(f"  {k:3s} {fmt(times[k])} ms" + (f"   {total / quartiles(times[k])[0] / 1e6:7.2f} G frames/s" if k != "B" else f"   {sum(fB) / quartiles(times[k])[0] / 1e6:7.2f} G frames/s (its own {sum(fB)} frames)"))
                print(f"  A/C {ratio(times['A'], times['C'])}   S/B {ratio(times['S'], times['B'])}   A/S {ratio(times['A'], times['S'])}   A'/A {ratio(times[chr(65) + chr(39)], times['A'])}")
            mel.close()
            del out, outB, gmax
        del pcm, xc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
