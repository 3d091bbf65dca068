#!/usr/bin/env python3
"""int16 PCM in / f16, bf16 rows out against the f32 call and against the status quo, in one process on one GPU (profiles/io_dtypes.txt).

Shapes: BASELINE config 2 (1024 x 10 s, 80 mels) and config 4 reduced to what fits beside the alternatives (1024 x 30 s, 128 mels), noise,
default precision mode.  Variants, timed with device events, alternating over --rounds rounds of --calls calls after a warm-up:
  A  the existing f32 call                              B  (S16, F32)      C  (F32, F16)      D  (S16, F16)      E  (S16, BF16)
  S  the status quo of a caller who holds int16 and wants f16: pcm16.to(float32).mul_(2**-15), call A, .to(float16) -- all on the device,
     all inside the timed window, on the same stream
Per variant: the median of the rounds, their spread (max - min), the algorithmic bytes per frame (hop x sample size + n_mels x row size) and
the fraction of the 8 TB/s HBM peak those bytes amount to at the measured time -- each variant on its OWN bytes: 480 B per frame for D is a
harder roofline than 960 B for A, so equal times mean half the fraction.

  python tools/io_bench.py [--out profiles/io_dtypes.txt]
  rocprofv3 --kernel-trace --stats -d DIR -- python tools/io_bench.py --rounds 1 --calls 20 --out /dev/null      (a separate run)
  python tools/io_bench.py --append-stats DIR --out profiles/io_dtypes.txt                                        (its summary, appended)"""
import argparse
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBS = 8000.0
HOP = 160


def append_stats(directory, out):
    files = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    rows = list(csv.DictReader(open(files[-1])))
    with open(out, "a") as fh:
        fh.write("\n# rocprofv3 --kernel-trace --stats, a separate run (--rounds 1 --calls 20): kernels by total time\n")
        fh.write(f"# {'calls':>6s} {'avg us':>9s} {'min us':>9s} {'max us':>9s} {'%':>6s}  kernel\n")
        for r in rows[:24]:
            num = lambda k: float(r.get(k) or 0.0)
            fh.write(f"  {int(num('Calls')):6d} {num('AverageNs') / 1e3:9.1f} {num('MinNs') / 1e3:9.1f} {num('MaxNs') / 1e3:9.1f} "
                     f"{num('Percentage'):6.2f}  {(r.get('Name') or '?')[:150]}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "io_dtypes.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--append-stats", default=None)
    args = ap.parse_args()
    if args.append_stats:
        return append_stats(args.append_stats, args.out)

    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd.hip import OUT_BF16, OUT_F16, OUT_F32, PCM_F32, PCM_S16
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lines = [f"# tools/io_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {args.rounds} rounds x {args.calls} calls per variant, alternating, after {args.warmup} warm-up calls each; device events; ms per call",
             "# frac = algorithmic bytes of the variant itself / time / 8 TB/s: D's 480 B per frame is a harder roofline than A's 960 B"]
    verdicts = []
    for name, n_clips, seconds, nm in (("config 2 (1024 x 10 s, 80 mels)", 1024, 10, 80), ("config 4 reduced (1024 x 30 s, 128 mels)", 1024, 30, 128)):
        n = seconds * 16000
        mel = M.HipMelSpectrogram(400, HOP, 16000.0, nm, device=0)
        mel.set_precision("auto")
        nf = mel.num_frames(n)
        gen = torch.Generator(device=dev).manual_seed(1234 + nm)
        pcm16 = torch.randint(-32768, 32768, (n_clips, n), generator=gen, device=dev, dtype=torch.int32)
        pcm16 = (pcm16 >> (torch.arange(n_clips, device=dev, dtype=torch.int32) & 7)[:, None]).to(torch.int16).contiguous()
        pcm32 = pcm16.to(torch.float32).mul_(2.0 ** -15)
        out32 = torch.empty((n_clips, nf, nm), device=dev, dtype=torch.float32)
        out16 = torch.empty((n_clips, nf, nm), device=dev, dtype=torch.int16)

        def call_a(src=None):
            mel.compute_uniform_device((pcm32 if src is None else src).data_ptr(), n, n, n_clips, out32.data_ptr(), stream)

        def status_quo():
            tmp = pcm16.to(torch.float32).mul_(2.0 ** -15)
            call_a(tmp)
            return out32.to(torch.float16)

        def io(pcm, out):
            src = pcm16 if pcm == PCM_S16 else pcm32
            dst = out32 if out == OUT_F32 else out16
            return lambda: mel.compute_uniform_device_io(src.data_ptr(), pcm, n, n, n_clips, dst.data_ptr(), out, stream)

        variants = [("A (F32, F32)  existing call", call_a, 4, 4), ("B (S16, F32)", io(PCM_S16, OUT_F32), 2, 4), ("C (F32, F16)", io(PCM_F32, OUT_F16), 4, 2),
                    ("D (S16, F16)", io(PCM_S16, OUT_F16), 2, 2), ("E (S16, BF16)", io(PCM_S16, OUT_BF16), 2, 2),
                    ("S status quo: to(f32) * 2^-15, A, to(f16)", status_quo, 2 + 4 + 4, 4 + 4 + 2)]
        # D == the status quo's result, bit for bit, before anything is timed
        io(PCM_S16, OUT_F16)()
        want = status_quo()
        torch.cuda.synchronize()
        assert torch.equal(out16.view(torch.float16), want), "D != the status quo's result"
        for _, fn, _, _ in variants:
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {v[0]: [] for v in variants}
        for _ in range(args.rounds):
            for label, fn, _, _ in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                ms[label].append(e0.elapsed_time(e1) / args.calls)
        frames = n_clips * nf
        lines += ["", f"## {name}: {frames} frames per call, default precision mode, int16 noise scaled per clip by 2^-(clip & 7)",
                  f"# {'variant':46s} {'median ms':>10s} {'spread ms':>10s} {'rounds (ms)':>44s} {'B/frame':>8s} {'GB/s':>8s} {'frac':>6s} {'G frames/s':>10s}"]
        med, spread = {}, {}
        for label, _, ib, ob in variants:
            r = ms[label]
            med[label], spread[label] = statistics.median(r), max(r) - min(r)
            bpf = HOP * ib + nm * ob
            gbs = frames * bpf / (med[label] * 1e-3) / 1e9
            lines.append(f"  {label:46s} {med[label]:10.4f} {spread[label]:10.4f} {' '.join(f'{x:.4f}' for x in r):>44s} {bpf:8d} {gbs:8.1f} {gbs / HBM_PEAK_GBS:6.3f} "
                         f"{frames / (med[label] * 1e-3) / 1e9:10.3f}")
        a, d, s = variants[0][0], variants[3][0], variants[5][0]
        run_spread = max(spread.values())
        verdicts.append(f"{name}: D {med[d]:.4f} ms against S {med[s]:.4f} ms: D is {med[s] / med[d]:.2f} x faster, the difference {med[s] - med[d]:.4f} ms "
                        f"{'exceeds' if med[s] - med[d] > run_spread else 'DOES NOT exceed'} the largest spread of the rounds ({run_spread:.4f} ms)")
        for label, _, _, _ in variants[1:5]:
            delta = med[label] - med[a]
            tol = max(spread[label], spread[a])
            verdicts.append(f"{name}: {label.split('(')[0].strip()} - A = {delta:+.4f} ms ({100 * delta / med[a]:+.1f} %): "
                            + ("faster than A" if delta < 0 else "within the spread of A" if delta <= tol else f"SLOWER than A beyond the spread ({tol:.4f} ms)"))
        mel.close()
        del pcm16, pcm32, out32, out16
    lines += ["", "## the two conditions, against the numbers above"] + ["# " + v for v in verdicts]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
