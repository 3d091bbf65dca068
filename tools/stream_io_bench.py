#!/usr/bin/env python3
"""Streaming bank: int16 PCM chunks in / f16 rows out against the f32 push and against the status quo, in one process on one GPU
(profiles/stream_io_dtypes.txt).  The sibling of tools/fbank_io_bench.py.

Shape: 4096 live streams x one hop (160 samples) per push, 400 / 160 / 80, default precision mode, noise: one row per stream and push.
Every push call returns after its launches have completed, so a push is timed on the host clock around the call; a bank per variant
(the steady-state plan cache is the bank's), all on one context.  --rounds rounds of --calls pushes per variant after a warm-up that
also takes every stream past its first window; a round times every variant once, even rounds in the order A B D, odd rounds reversed.

Host form (chunks and rows in host memory):
  A  melspec_stream_push_host on f32 chunks
  B  the status quo of a caller who holds int16 and wants f16: chunk.astype(float32) * 2^-15 on the host, call A, rows.astype(float16)
     on the host -- all inside the timed window
  D  (S16, F16) through melspec_stream_push_host_io
Device form (chunks and rows in device memory):
  A  melspec_stream_push_device: the f32 chunks are already in the bank's slots (melspec_stream_input_ptr), nothing is copied
  B  the status quo of a device producer that holds int16: convert into the slots (to(float32) * 2^-15, one strided write), call A,
     rows.to(float16) -- on the device, inside the timed window
  D  (S16, F16) through melspec_stream_push_device_io with d_chunks = the int16 buffer
Per variant: the median of the rounds' mean push time and their spread (max - min), and the bytes that cross the bus (host form) or are
read and written by the caller's side of the push (device form).  The claim to confirm or refute: D faster than B.

  python tools/stream_io_bench.py [--out profiles/stream_io_dtypes.txt]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Raw:
    """device memory the library owns, as a strided array torch can wrap"""

    def __init__(self, ptr, shape, strides, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "strides": strides, "typestr": typestr, "data": (ptr, False), "version": 2}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_io_dtypes.txt"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=8)
    args = ap.parse_args()

    import numpy as np
    import torch
    import mel_spec_amd as M
    from mel_spec_amd import build as hip_build
    from mel_spec_amd._lib import lib as load
    from mel_spec_amd.hip import OUT_F16, PCM_S16
    lib = load()
    dev = torch.device("cuda:0")
    n, hop, nm = 4096, 160, 80
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    rng = np.random.default_rng(4321)
    pcm16 = (rng.integers(-32768, 32768, (n, hop), dtype=np.int32) >> (np.arange(n, dtype=np.int32) & 7)[:, None]).astype(np.int16)
    pcm32 = pcm16.astype(np.float32) * np.float32(2.0 ** -15)
    ids, lens, frames = np.arange(n, dtype=np.uint32), np.full(n, hop, np.uint32), np.zeros(n, np.uint32)
    ip, lp, fp = ids.ctypes.data_as(u32p), lens.ctypes.data_as(u32p), frames.ctypes.data_as(u32p)
    mel = M.HipMelSpectrogram(400, hop, 16000.0, nm, device=0)
    banks = {k: M.StreamBank(mel, n, hop) for k in ("hA", "hB", "hD", "dA", "dB", "dD")}
    assert banks["hD"].supports_io(PCM_S16, OUT_F16)
    rows32, rows16 = np.zeros((n, nm), np.float32), np.zeros((n, nm), np.float16)

    def ok(rc):
        assert rc == 0, lib.melspec_last_error()

    # ---- host form
    def host_a(bank="hA", src=pcm32):
        ok(lib.melspec_stream_push_host(banks[bank]._h, ip, src.ctypes.data_as(f32p), lp, n, rows32.ctypes.data_as(f32p), rows32.size, fp))

    def host_b():
        host_a("hB", pcm16.astype(np.float32) * np.float32(2.0 ** -15))
        return rows32.astype(np.float16)

    def host_d():
        ok(lib.melspec_stream_push_host_io(banks["hD"]._h, ip, pcm16.ctypes.data_as(C.c_void_p), PCM_S16, lp, n, rows16.ctypes.data_as(C.c_void_p), OUT_F16,
                                           rows16.size, fp))

    # ---- device form
    d16 = torch.from_numpy(pcm16).to(dev)
    out32 = torch.empty((n, nm), device=dev, dtype=torch.float32)
    out16 = torch.empty((n, nm), device=dev, dtype=torch.float16)

    def slots(bank):
        p0 = bank.input_ptr(0)
        return torch.as_tensor(_Raw(p0, (n, hop), (bank.input_ptr(1) - p0, 4), "<f4"), device=dev)

    slots_a, slots_b = slots(banks["dA"]), slots(banks["dB"])
    slots_a.copy_(torch.from_numpy(pcm32).to(dev))
    torch.cuda.synchronize()

    def dev_a(bank="dA"):
        ok(lib.melspec_stream_push_device(banks[bank]._h, ip, lp, n, C.c_void_p(out32.data_ptr()), None, fp, None))

    def dev_b():
        slots_b.copy_(d16.to(torch.float32).mul_(2.0 ** -15))
        torch.cuda.synchronize()                 # the push runs on the bank's own stream
        dev_a("dB")
        res = out32.to(torch.float16)
        torch.cuda.synchronize()
        return res

    def dev_d():
        ok(lib.melspec_stream_push_device_io(banks["dD"]._h, ip, C.c_void_p(d16.data_ptr()), PCM_S16, None, lp, n, C.c_void_p(out16.data_ptr()), OUT_F16,
                                             None, fp, None))

    def measure(variants):
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
        return ms

    host = [("A", host_a), ("B", host_b), ("D", host_d)]
    device = [("A", dev_a), ("B", dev_b), ("D", dev_d)]
    for _ in range(4):                           # past the first window; then B and D must agree bit for bit, before anything is timed
        want_h = host_b(); host_d()
        want_d = dev_b(); dev_d()
    torch.cuda.synchronize()
    assert frames.sum() == n and np.array_equal(rows16.view(np.uint16), want_h.view(np.uint16)), "host D != the status quo's result"
    assert torch.equal(out16, want_d), "device D != the status quo's result"
    ms_h, ms_d = measure(host), measure(device)

    per = n * hop
    bus = {"A": per * 4 + n * nm * 4, "B": per * 4 + n * nm * 4, "D": per * 2 + n * nm * 2}
    hbm = {"A": n * nm * 4, "B": (per * 2 + per * 4) + n * nm * 4 + (n * nm * 4 + n * nm * 2), "D": per * 2 + n * nm * 2}
    what_h = {"A": "push_host on f32", "B": "status quo: astype(f32) * 2^-15, A, astype(f16), on the host", "D": "(S16, F16) through push_host_io"}
    what_d = {"A": "push_device, f32 already in the slots", "B": "status quo: to(f32) * 2^-15 into the slots, A, to(f16), on the device",
              "D": "(S16, F16) through push_device_io, d_chunks = the int16 buffer"}
    lines = [f"# tools/stream_io_bench.py -- {torch.cuda.get_device_name(0)}, library source hash {hip_build.source_hash()}",
             f"# {n} streams x one hop ({hop} samples) per push, 400 / {hop} / {nm}, default mode: {n} rows per push; {args.rounds} rounds x {args.calls} pushes per "
             f"variant, order A B D and its reverse in turn, after {args.warmup} warm-up pushes each; host clock around the (synchronous) calls"]
    for title, ms, what, nbytes, col in (("host form", ms_h, what_h, bus, "bus B / push"), ("device form", ms_d, what_d, hbm, "caller's HBM B / push")):
        med = {k: statistics.median(v) for k, v in ms.items()}
        lines.append(f"# {title}: {'ms / push':>9s} {'spread':>7s} {'rows / s':>11s} {col:>22s}")
        for k in "ABD":
            lines.append(f"  {k} {med[k]:20.4f} {max(ms[k]) - min(ms[k]):7.4f} {n / (med[k] * 1e-3):11.4e} {nbytes[k]:22d}   {what[k]}")
        lines.append(f"# {title}: B / D = {med['B'] / med['D']:.2f}, D / A = {med['D'] / med['A']:.2f}: D is " +
                     ("faster than B" if med["D"] < med["B"] else "NOT faster than B") + ", " + ("faster than A" if med["D"] < med["A"] else "slower than A"))
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out != os.devnull:
        with open(args.out, "w") as fh:
            fh.write(text)
    for b in banks.values():
        b.close()
    mel.close()


if __name__ == "__main__":
    main()
