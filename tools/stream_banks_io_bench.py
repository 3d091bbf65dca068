#!/usr/bin/env python3
"""Kaldi and NeMo / Parakeet stream banks: f16 rows straight out of the push (melspec_*_stream_push_device_io) against what a caller
did before -- the f32 push and a cast kernel of its own over every row --, in one process on one GPU (profiles/stream_banks_io.txt).
Recorded, not gated.

Shape (tools/blm_stream_bench.py's): 1024 live streams, 16 kHz, 80 mels / bins, chunks of 10 ms, 100 ms and 1 s (160 / 1600 / 16000
samples) already in device memory, noise; the Kaldi bank (f64) and the NeMo bank in the default f64 mode and in MELSPEC_PRECISION_F32.
Per bank and chunk size, five variants, each on a bank of its own:
  A   the existing f32 push_device, chunks at *_stream_input_ptr
  B   the status quo for f16 rows: A, then a torch cast of the packed f32 rows to f16 on the same stream, then the synchronise
  Bs  the same for int16 chunks: a torch int16 -> f32 conversion (x 2^-15) of the chunks into a staging buffer in front, the f32 push
      with d_chunks = that buffer, the cast of the rows, the synchronise
  C   push_device_io (F32, F16), chunks at *_stream_input_ptr
  D   push_device_io (S16, F16), d_chunks = the int16 chunks
Every variant returns after its work has completed (the pushes by contract, B / Bs by the synchronise), so a call is timed on the host
clock around it.  --rounds rounds of --calls calls per variant after --warmup calls each (which also take every stream past its first
frame); a round times every variant once, even rounds in the order A B Bs C D, odd rounds reversed.  Per variant: the median of the rounds'
mean call time and their spread (max - min).

  python tools/stream_banks_io_bench.py [--out profiles/stream_banks_io.txt]"""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_banks_io.txt"))
    ap.add_argument("--streams", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=6)
    args = ap.parse_args()

    import numpy as np
    import torch   # before libmelspec_hip.so is loaded
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd._lib import lib as load
    lib = load()
    assert M.device_count() >= 1 and torch.cuda.is_available(), "no GPU: nothing to measure"
    n, nm, hop = args.streams, 80, 160
    rng = np.random.default_rng(4321)
    ids = np.arange(n, dtype=np.uint32)
    order = ["A", "B", "Bs", "C", "D"]
    lines = [f"# tools/stream_banks_io_bench.py -- library source hash {hip_build.source_hash()}",
             f"# {n} streams, 16 kHz, {nm} mels / bins; {args.rounds} rounds x {args.calls} calls per variant, order {' '.join(order)} and its reverse in turn, after "
             f"{args.warmup} warm-up calls each; host clock around calls that return after their work has completed",
             "# A f32 push_device   B A + torch cast of the rows to f16 + synchronize   Bs torch int16 -> f32 of the chunks + B   C push_device_io (F32, F16)   D push_device_io (S16, F16)",
             f"# {'bank':>9s} {'chunk':>7s} {'rows/push':>10s} | " + " | ".join(f"{k + ' ms':>8s} {'spread':>7s}" for k in order) + f" | {'C / B':>6s} {'D / Bs':>6s} {'C / A':>6s}"]
    stream = torch.cuda.Stream()                     # the pushes and torch's kernels share it
    torch.cuda.set_stream(stream)
    s_ptr = stream.cuda_stream
    assert s_ptr
    for bank_name, mode in (("kaldi", None), ("nemo", "f64"), ("nemo", "f32")):
        if bank_name == "kaldi":
            obj, make = M.Fbank(M.FbankConfig()), M.FbankStreamBank
        else:
            obj, make = M.BatchLogMelSpectrogram(M.BatchLogMelConfig()), M.BlmStreamBank
            obj.set_precision(mode)
            assert obj.precision == mode
        for chunk in (160, 1600, 16000):
            lens = np.full(n, chunk, np.uint32)
            rows = chunk // hop                      # per stream and push in steady state
            pcm16 = rng.integers(-3277, 3277, (n, chunk), dtype=np.int16)
            pcm32 = pcm16.astype(np.float32) * np.float32(2.0 ** -15)
            banks = {k: make(obj, n, chunk) for k in order}
            for k in ("A", "B", "C"):                # the chunks stay where a push leaves them: written once
                p0 = banks[k].input_ptr(0)
                step = banks[k].input_ptr(1) - p0 if n > 1 else 0
                for s in range(n):
                    c = np.ascontiguousarray(pcm32[s])
                    assert lib.melspec_memcpy_h2d(C.c_void_p(p0 + s * step), c.ctypes.data_as(C.c_void_p), c.nbytes) == 0
            d16 = torch.from_numpy(pcm16).cuda()
            stage32 = torch.empty((n, chunk), dtype=torch.float32, device="cuda")
            out32 = torch.empty(n * rows * nm, dtype=torch.float32, device="cuda")
            out16 = torch.empty(n * rows * nm, dtype=torch.float16, device="cuda")
            torch.cuda.synchronize()

            def run_a():
                banks["A"].push_device(ids, lens, out32.data_ptr(), stream=s_ptr)

            def run_b():
                banks["B"].push_device(ids, lens, out32.data_ptr(), stream=s_ptr)
                out16.copy_(out32)
                stream.synchronize()

            def run_bs():
                torch.mul(d16, 2.0 ** -15, out=stage32)
                banks["Bs"].push_device(ids, lens, out32.data_ptr(), d_chunks=stage32.data_ptr(), pcm_dtype=M.hip.PCM_F32, stream=s_ptr)
                out16.copy_(out32)
                stream.synchronize()

            def run_c():
                banks["C"].push_device_io(ids, 0, M.hip.PCM_F32, lens, out16.data_ptr(), M.hip.OUT_F16, stream=s_ptr)

            def run_d():
                banks["D"].push_device_io(ids, d16.data_ptr(), M.hip.PCM_S16, lens, out16.data_ptr(), M.hip.OUT_F16, stream=s_ptr)

            variants = list(zip(order, (run_a, run_b, run_bs, run_c, run_d)))
            for _ in range(args.warmup):
                for _, fn in variants:
                    fn()
            ms = {k: [] for k in order}
            for r in range(args.rounds):
                for label, fn in (variants if r % 2 == 0 else variants[::-1]):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        fn()
                    ms[label].append((time.perf_counter() - t0) * 1e3 / args.calls)
            med = {k: statistics.median(v) for k, v in ms.items()}
            spread = {k: max(v) - min(v) for k, v in ms.items()}
            lines.append(f"  {bank_name + ('' if mode is None else ' ' + mode):>9s} {chunk:7d} {n * rows:10d} | " + " | ".join(f"{med[k]:8.4f} {spread[k]:7.4f}" for k in order) +
                         f" | {med['C'] / med['B']:6.2f} {med['D'] / med['Bs']:6.2f} {med['C'] / med['A']:6.2f}")
            for b in banks.values():
                b.close()
            del d16, stage32, out32, out16
        obj.close()
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
