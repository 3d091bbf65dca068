"""The streaming bank with 16-bit ends: int16 PCM chunks in, f16 / bf16 rows out (melspec_stream_supports_io / _push_host_io /
_flush_host_io / _push_device_io).

The yardsticks are those of tests/test_io_dtypes.py and just as exact:
  * the bank's state stays f32 and an int16 sample is int16 * 2^-15 exactly, converted where the chunk is scattered into the state: a bank
    driven through the _io calls must emit THE BITS of a twin bank -- a second context of the same settings -- driven by the existing
    melspec_stream_push_host / _flush_host on `chunk.astype(float32) * float32(2**-15)`, push by push, frames_out included;
  * an f16 / bf16 row is the round-to-nearest-even of the f32 row of the twin's push (round_to);
  * against the oracle's streaming loop the gate is the mode's existing gate + half a unit in the last place of the 16-bit type for rows in
    [-1.5, 2) (MODE_TOL + HALF_ULP), and the test asserts that range.

Every output, host or device, is the middle of an allocation filled with the type's sentinel (a NaN with a payload no kernel computes),
with a guard band on each side; device pushes also use odd element offsets and gaps between the streams' rows.  Bands and gaps must
still hold the sentinel afterwards and every element of the output proper must have been written; after a refused call ALL of it is
the sentinel."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_io_dtypes import (ERR_CAPACITY, ERR_INVALID_ARG, ERR_UNSUPPORTED, HALF_ULP, MODE_TOL, NEW_COMBOS, OUT_BF16, OUT_F16, OUT_F32, OUT_NP,
                            PCM_F32, PCM_S16, SENTINEL, s16_extremes, s16_noise, s16_speech, s16_tone, round_to, to_f32, to_f64)

SR = 16000.0
GUARD = 512                                     # elements of guard band on each side of an output
SIZES = [0, 1, 159, 160, 161, 320, 399, 400, 401, 1000]
STREAM_IO_SYMBOLS = ["melspec_stream_supports_io", "melspec_stream_push_host_io", "melspec_stream_flush_host_io", "melspec_stream_push_device_io"]
u32p, u64p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)
PCM_NP = {PCM_F32: np.float32, PCM_S16: np.int16}


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


# ---- inputs and push schedules -----------------------------------------------------------------------------------------------------

def sources(jfk, n_streams, n=8000):
    """int16 input per stream: noise, speech (the fixture scaled to peak 0.9), tone over a floor, the two extremes alternating, ...; the
    lengths differ so that the streams run dry at different pushes"""
    make = [lambda s, k: s16_noise(s, k), lambda s, k: s16_speech(jfk, s, k), lambda s, k: s16_tone(s, k), lambda s, k: s16_extremes(2 * s, k)]
    return [make[s % 4](s, n + 37 * s) for s in range(n_streams)]


def schedule(totals, max_chunk, seed):
    """[(ids, lens)]: each push goes to a random subset of the live streams with chunk sizes from SIZES or random ones (tests/test_stream.py:
    _drive), so that the chunks staged back to back start at odd elements"""
    rng = np.random.default_rng(seed)
    pos, live, pushes = [0] * len(totals), set(range(len(totals))), []
    while live:
        ids = [s for s in sorted(live) if rng.random() < 0.7]
        if not ids:
            continue
        lens = []
        for s in ids:
            n = int(rng.choice(SIZES)) if rng.random() < 0.5 else int(rng.integers(0, max_chunk + 1))
            n = min(n, max_chunk, totals[s] - pos[s])
            lens.append(n); pos[s] += n
            if pos[s] >= totals[s]:
                live.discard(s)
        pushes.append((ids, lens))
    starts = np.concatenate([np.cumsum([0] + ln[:-1]) for _, ln in pushes])
    assert (starts & 1).sum() * 8 >= starts.size, "the schedule should stage chunks at odd elements"
    return pushes


# ---- fenced outputs ----------------------------------------------------------------------------------------------------------------

class HostFence:
    def __init__(self, n, out):
        self.n, self.s = int(n), OUT_NP[out](SENTINEL[out])
        self.raw = np.full(self.n + 2 * GUARD, self.s, OUT_NP[out])
        self.ptr = C.c_void_p(self.raw.ctypes.data + GUARD * self.raw.itemsize)

    def untouched(self):
        return bool(np.all(self.raw == self.s))

    def bits(self, written):
        """the first `written` elements, all of them written; everything else -- bands and the unused tail -- still the sentinel"""
        lo, body, hi = self.raw[:GUARD], self.raw[GUARD:GUARD + written], self.raw[GUARD + written:]
        assert np.all(lo == self.s), f"write below the output: {int(np.sum(lo != self.s))} elements"
        assert np.all(hi == self.s), f"write past the {written} elements of the output: {int(np.sum(hi != self.s))} elements"
        assert not np.any(body == self.s), f"{int(np.sum(body == self.s))} of {written} output elements never written"
        return body.copy()


class DevFence:
    """device memory for `n` elements of any row type (sized for f32) between two guard bands; arm(out) fills all of it with out's sentinel"""

    def __init__(self, gpu, n):
        self.n = int(n)
        self.buf = gpu.DeviceBuffer((self.n + 2 * GUARD) * 4)
        self.ptr = self.buf.ptr + GUARD * 4

    def arm(self, out):
        self.out = out
        self.buf.upload(np.full(self.buf.nbytes // np.dtype(OUT_NP[out]).itemsize, SENTINEL[out], OUT_NP[out]))
        return self

    def raw(self):
        """(elements below ptr, elements from ptr on) in the armed type"""
        es = np.dtype(OUT_NP[self.out]).itemsize
        a = self.buf.download(self.buf.nbytes // es, OUT_NP[self.out])
        return a[:GUARD * 4 // es], a[GUARD * 4 // es:]

    def untouched(self):
        lo, rest = self.raw()
        return bool(np.all(lo == SENTINEL[self.out]) and np.all(rest == SENTINEL[self.out]))

    def rows(self, offs, counts):
        """the pieces [offs[i], offs[i] + counts[i]) from ptr on, all written; every other element still the sentinel"""
        lo, rest = self.raw()
        s = OUT_NP[self.out](SENTINEL[self.out])
        assert np.all(lo == s), f"write below the output: {int(np.sum(lo != s))} elements"
        mask = np.zeros(rest.size, bool)
        res = []
        for o, k in zip(offs, counts):
            o, k = int(o), int(k)
            assert o + k <= self.n
            piece = rest[o:o + k]
            assert not np.any(piece == s), f"{int(np.sum(piece == s))} of {k} elements at offset {o} never written"
            mask[o:o + k] = True
            res.append(piece.copy())
        stray = (rest != s) & ~mask
        assert not stray.any(), f"{int(stray.sum())} elements outside the rows were written (gaps / upper band), first at {int(np.argmax(stray))}"
        return res


# ---- the calls ---------------------------------------------------------------------------------------------------------------------

class Bank:
    """a bank over a context of its own, driven through the C ABI"""

    def __init__(self, gpu, geo, mode, n_streams, max_chunk):
        self.gpu, self.lib = gpu, gpu._lib.lib()
        self.m = gpu.HipMelSpectrogram(geo[0], geo[1], SR, geo[2])
        if mode is not None:
            self.m.set_precision(mode)
        self.nm, self.n_streams = geo[2], n_streams
        self.bank = gpu.StreamBank(self.m, n_streams, max_chunk)
        self.h = self.bank._h

    def close(self):
        self.bank.close(); self.m.close()          # both idempotent

    def after(self, ids, lens):
        return [self.bank.frames_after(int(s), int(n)) for s, n in zip(ids, lens)]

    def state(self):
        """what a refused or failed call must leave alone, as far as the ABI shows it"""
        return [self.bank.frames_after(s, n) for s in range(self.n_streams) for n in (0, 1, 159, 160, 400)]

    def push_host(self, ids, chunks, pcm=PCM_F32, out=OUT_F32, plain=False, flush=False, expect=0, cap_delta=0, null=None):
        """-> (frames_out, bits of the rows) -- or, expect != 0, asserts the status and that output and frames_out are untouched"""
        ids = _u32(ids)
        lens = _u32([len(c) for c in chunks])
        dt = PCM_NP.get(pcm, np.int16)              # an unknown code: the call must fail before it looks at the buffers
        flat = np.ascontiguousarray(np.concatenate(chunks) if len(chunks) else [], dt)
        flat = flat if flat.size else np.zeros(1, dt)
        cap = (len(ids) if flush else sum(self.after(ids, lens))) * self.nm + cap_delta
        f = HostFence(cap, out if out in OUT_NP else OUT_F16)
        frames = np.full(len(ids), 0xABCD, np.uint32)
        src, dst = (None if null == "samples" else _vp(flat)), (None if null == "out" else f.ptr)
        if plain:
            assert pcm == PCM_F32 and out == OUT_F32
            src32, dst32 = C.cast(src, f32p), C.cast(dst, f32p)
            rc = (self.lib.melspec_stream_flush_host(self.h, ids.ctypes.data_as(u32p), len(ids), dst32, cap, frames.ctypes.data_as(u32p)) if flush else
                  self.lib.melspec_stream_push_host(self.h, ids.ctypes.data_as(u32p), src32, lens.ctypes.data_as(u32p), len(ids), dst32, cap,
                                                    frames.ctypes.data_as(u32p)))
        elif flush:
            rc = self.lib.melspec_stream_flush_host_io(self.h, ids.ctypes.data_as(u32p), len(ids), dst, out, cap, frames.ctypes.data_as(u32p))
        else:
            rc = self.lib.melspec_stream_push_host_io(self.h, ids.ctypes.data_as(u32p), src, pcm, lens.ctypes.data_as(u32p), len(ids), dst, out, cap,
                                                      frames.ctypes.data_as(u32p))
        assert rc == expect, (rc, expect, self.lib.melspec_last_error())
        if expect:
            assert f.untouched() and np.all(frames == 0xABCD), "a failing call wrote into its output"
            return None
        assert flush or int(frames.sum()) * self.nm == cap
        return frames, f.bits(int(frames.sum()) * self.nm)

    def push_device(self, fence, ids, lens, d_chunks, pcm, out, src_off=None, out_off=None, expect=0):
        """-> frames_out; the rows are in `fence` (armed by the caller)"""
        ids, lens = _u32(ids), _u32(lens)
        frames = np.full(len(ids), 0xABCD, np.uint32)
        so = None if src_off is None else np.ascontiguousarray(src_off, np.uint64)
        oo = None if out_off is None else np.ascontiguousarray(out_off, np.uint64)
        rc = self.lib.melspec_stream_push_device_io(self.h, ids.ctypes.data_as(u32p), C.c_void_p(d_chunks), pcm, None if so is None else so.ctypes.data_as(u64p),
                                                    lens.ctypes.data_as(u32p), len(ids), None if fence is None else C.c_void_p(fence.ptr), out,
                                                    None if oo is None else oo.ctypes.data_as(u64p), frames.ctypes.data_as(u32p), None)
        assert rc == expect, (rc, expect, self.lib.melspec_last_error())
        if expect:
            assert (fence is None or fence.untouched()) and np.all(frames == 0xABCD), "a failing call wrote into its output"
            return None
        return frames


@pytest.fixture
def banks(gpu):
    """Bank(...) factory; every bank is closed in front of its context at teardown, also when the test failed (a bank must not outlive
    its context, and the garbage collector knows no order)"""
    made = []

    def make(geo, mode, n_streams, max_chunk):
        made.append(Bank(gpu, geo, mode, n_streams, max_chunk))
        return made[-1]

    yield make
    for b in reversed(made):
        b.close()


def drive(bank, src, pushes, pcm, out, plain=False):
    """the whole schedule and a final flush of every stream -> [(frames_out, bits)] per push"""
    pos, res = [0] * len(src), []
    for ids, lens in pushes:
        chunks = [src[s][pos[s]:pos[s] + n] for s, n in zip(ids, lens)]
        for s, n in zip(ids, lens):
            pos[s] += n
        res.append(bank.push_host(ids, chunks, pcm, out, plain))
    assert pos == [len(x) for x in src]
    res.append(bank.push_host(list(range(len(src))), [src[0][:0]] * len(src), PCM_F32 if plain else pcm, out, plain, flush=True))
    return res


def same_pushes(got, want32, out, what):
    assert len(got) == len(want32)
    for k, ((fg, bg), (fw, bw)) in enumerate(zip(got, want32)):
        assert np.array_equal(fg, fw), f"{what}: push {k}: frames_out {fg} != the twin's {fw}"
        want = round_to(bw, out)
        diff = bg != want
        assert not diff.any(), f"{what}: push {k}: {int(diff.sum())} of {diff.size} elements differ from the twin's (rounded) bits, first at " \
                               f"{int(np.argmax(diff))}: {bg[np.argmax(diff)]:#x} != {want[np.argmax(diff)]:#x}"


def per_stream(n_streams, pushes, res, nm):
    """the rows of every push handed to their streams, in order (the last entry of res is the flush of all streams)"""
    rows = [[] for _ in range(n_streams)]
    for (ids, _), (frames, bits) in zip(list(pushes) + [(list(range(n_streams)), None)], res):
        cur = 0
        for s, f in zip(ids, frames):
            rows[s].append(bits[cur:cur + int(f) * nm].reshape(int(f), nm)); cur += int(f) * nm
    return [np.concatenate(r) for r in rows]


# ---- 1. twin banks, bit for bit ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32", "auto"])
@pytest.mark.parametrize("nm", [80, 128])
def test_twin_banks_bit_for_bit(gpu, banks, jfk, mode, nm):
    """Bank A: push_host / flush_host on the converted f32 chunks.  Bank B, on a second context of the same settings (a fresh bank per
    combination): the _io calls on the same pushes -- 5 streams, max_chunk 1000, ~8000 int16 samples each, chunk sizes 0, 1, 159, 160, 161,
    320, 399, 400, 401, 1000 and random ones to random subsets of the streams, a flush at the end.  For the five new (pcm, out) pairs every
    row of every push is round_to(A's rows, out) and every frames_out is A's; (F32, F32) through _io is the plain call."""
    geo = (400, 160, nm)
    s16 = sources(jfk, 5)
    f32 = [to_f32(x) for x in s16]
    pushes = schedule([len(x) for x in s16], 1000, 11)
    a = banks(geo, mode, 5, 1000)
    want = drive(a, f32, pushes, PCM_F32, OUT_F32, plain=True)
    assert sum(int(f.sum()) for f, _ in want) > 5 * 45
    b = banks(geo, mode, 5, 1000)
    for pcm, out in [(PCM_F32, OUT_F32)] + NEW_COMBOS:
        assert b.bank.supports_io(pcm, out)
        b.bank.close()
        b.bank = gpu.StreamBank(b.m, 5, 1000); b.h = b.bank._h
        got = drive(b, s16 if pcm == PCM_S16 else f32, pushes, pcm, out)
        same_pushes(got, want, out, f"({pcm}, {out}) {mode} {nm}")


# ---- 2. against the oracle ---------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32", "auto"])
@pytest.mark.parametrize("nm", [80, 128])
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
def test_s16_chunks_16bit_rows_against_the_oracle(gpu, banks, oracle, jfk, mode, nm, out):
    """(S16, F16) and (S16, BF16): each stream's concatenated rows against oracle.stream_mel on the exactly converted input, flush
    included.  Gate = the mode's gate against the oracle + half a unit in the last place of the row type for rows in [-1.5, 2)."""
    s16 = sources(jfk, 5)
    pushes = schedule([len(x) for x in s16], 1000, 12)
    b = banks((400, 160, nm), mode, 5, 1000)
    rows = per_stream(5, pushes, drive(b, s16, pushes, PCM_S16, out), nm)
    gate, worst, lo, hi = MODE_TOL[mode] + HALF_ULP[out], 0.0, np.inf, -np.inf
    for s in range(5):
        want = np.asarray(oracle.stream_mel(to_f32(s16[s]), 400, 160, nm, SR, flush_tail=True), np.float64)
        assert rows[s].shape == want.shape, (s, rows[s].shape, want.shape)
        d = np.abs(to_f64(rows[s], out) - want)
        d[np.isnan(d)] = np.inf
        worst, lo, hi = max(worst, float(d.max())), min(lo, float(want.min())), max(hi, float(want.max()))
    print(f"\nSTREAM-IO-ORACLE {mode} {nm} out={out}: worst {worst:.3e}, gate {gate:.3e}, oracle rows in [{lo:.3f}, {hi:.3f}]")
    assert -1.5 <= lo and hi < 2.0, "the half-ulp term assumes rows in [-1.5, 2)"
    assert worst <= gate, (worst, gate)


# ---- 3. device pushes --------------------------------------------------------------------------------------------------------------

def gapped(chunks, dtype):
    """the chunks in one flat buffer whose filler (12345) sits in gaps of 1 to 2 elements in front of every chunk, the gap chosen so that
    three chunks of four start at an odd element and the fourth at an even one -> (flat, offsets)"""
    offs, cur = [], 0
    for c, x in enumerate(chunks):
        cur += 1 + ((cur + 1) & 1 == (c % 4 == 3))
        offs.append(cur)
        cur += len(x)
    flat = np.full(cur + 3, 12345, dtype)
    for o, x in zip(offs, chunks):
        flat[o:o + len(x)] = x
    assert sum(o & 1 for o in offs) * 2 >= len(offs)
    return flat, np.array(offs, np.uint64)


def gapped_rows(frames, nm):
    """row offsets in elements: odd gaps in front of every stream's rows, so that the outputs alternate between odd and even offsets"""
    oo, cur = [], 0
    for c, f in enumerate(frames):
        cur += 1 + 2 * (c % 4)
        oo.append(cur)
        cur += int(f) * nm
    return np.array(oo, np.uint64), cur


@pytest.mark.gpu
@pytest.mark.parametrize("nm", [80, 128])
def test_device_pushes(gpu, banks, jfk, nm):
    """64 streams, bank B through melspec_stream_push_device_io against the twin's push_host on the converted chunks.
    (a) d_chunks: int16 (or f32) chunks of mixed sizes in a flat device buffer with filler in gaps of 1-2 elements (half the offsets odd),
        rows at odd out_offsets with gaps, every (pcm, out) pair in turn;
    (b) steady state: the same ids, one hop each, out dtype F32 / F16 / BF16 / F16 alternating into the same d_out ten times, then F16
        twice more (a typed plan replayed): every push has the bits of the twin's push of that step;
    (c) d_chunks == NULL: f32 written at input_ptr, F16 rows out; the same call with pcm_dtype = S16 is MELSPEC_ERR_INVALID_ARG."""
    n, hop = 64, 160
    geo = (400, hop, nm)
    a, b = banks(geo, None, n, 1000), banks(geo, None, n, 1000)
    s16 = sources(jfk, n, 10000)
    pos = [0] * n
    rng = np.random.default_rng(13)
    ids = list(range(n))
    fence = DevFence(gpu, n * 7 * nm + 8 * n + 64)

    def take(lens):
        chunks = [s16[s][pos[s]:pos[s] + k] for s, k in zip(ids, lens)]
        for s, k in zip(ids, lens):
            pos[s] += k
        return chunks

    def twin(chunks, out):
        fw, bw = a.push_host(ids, [to_f32(c) for c in chunks], plain=True)
        cur, rows = 0, []
        for f in fw:
            rows.append(round_to(bw[cur:cur + int(f) * nm], out)); cur += int(f) * nm
        return fw, rows

    def check(got, want, what):
        for s, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), f"{what}: stream {s}: {int((g != w).sum())} of {w.size} elements differ from the twin's (rounded) bits"

    # (a)
    for k, (pcm, out) in enumerate(NEW_COMBOS + [(PCM_F32, OUT_F32)]):
        lens = [int(rng.choice(SIZES)) if rng.random() < 0.6 else int(rng.integers(0, 1001)) for _ in ids]
        chunks = take(lens)
        fw, want = twin(chunks, out)
        flat, so = gapped(chunks if pcm == PCM_S16 else [to_f32(c) for c in chunks], PCM_NP[pcm])
        oo, total = gapped_rows(fw, nm)
        assert total <= fence.n and (k == 0 or int(fw.sum()) > n // 2)
        d = gpu.DeviceBuffer(flat.nbytes); d.upload(flat)
        fg = b.push_device(fence.arm(out), ids, lens, d.ptr, pcm, out, so, oo)
        assert np.array_equal(fg, fw), (k, fg, fw)
        check(fence.rows(oo, fw * nm), want, f"(a) push {k} ({pcm}, {out})")
        d.free()
    # every stream past its first window with nothing pending: the steady state of (b) can be cached
    lens = [2 * 400 + (-(pos[s] % hop)) % hop for s in ids]
    chunks = take(lens)
    fw, want = twin(chunks, OUT_F32)
    flat = np.concatenate(chunks)
    d = gpu.DeviceBuffer(flat.nbytes); d.upload(flat)
    oo, total = gapped_rows(fw, nm)
    fg = b.push_device(fence.arm(OUT_F32), ids, lens, d.ptr, PCM_S16, OUT_F32, None, oo)           # back to back: h_src_offsets == NULL
    assert np.array_equal(fg, fw)
    check(fence.rows(oo, fw * nm), want, "back-to-back chunks")
    d.free()
    # (b)
    d = gpu.DeviceBuffer(n * hop * 2)
    packed = np.arange(n) * nm
    for k, out in enumerate([OUT_F32, OUT_F16, OUT_BF16, OUT_F16] * 2 + [OUT_F32, OUT_F16, OUT_F16, OUT_F16]):
        chunks = take([hop] * n)
        fw, want = twin(chunks, out)
        assert np.all(fw == 1)
        d.upload(np.concatenate(chunks))
        fg = b.push_device(fence.arm(out), ids, [hop] * n, d.ptr, PCM_S16, out)
        assert np.array_equal(fg, fw)
        check(fence.rows(packed, fw * nm), want, f"(b) step {k} out {out}")
    d.free()
    # (c)
    def at_input_ptr(chunks):
        for s, c in zip(ids, chunks):
            x = to_f32(c)
            assert b.lib.melspec_memcpy_h2d(C.c_void_p(b.bank.input_ptr(s)), _vp(x), x.nbytes) == 0

    chunks = take([hop + 1] * n)
    at_input_ptr(chunks)
    before = b.state()
    b.push_device(fence.arm(OUT_F16), ids, [hop + 1] * n, None, PCM_S16, OUT_F16, expect=ERR_INVALID_ARG)
    assert b.state() == before
    fw, want = twin(chunks, OUT_F16)
    fg = b.push_device(fence, ids, [hop + 1] * n, None, PCM_F32, OUT_F16)
    assert np.array_equal(fg, fw)
    check(fence.rows(packed, fw * nm), want, "(c) chunks at input_ptr, F16 rows")
    fence.buf.free()


# ---- 4. other geometries -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(512, 160, 80), (400, 128, 40), (1024, 256, 80)], ids=["512-160-80", "400-128-40", "1024-256-80"])
def test_other_geometries_take_int16_and_refuse_16bit_rows(gpu, banks, jfk, geo):
    """The conversion is in the scatter: (S16, F32) equals the plain bank bit for bit on every geometry.  16-bit rows are refused with
    MELSPEC_ERR_UNSUPPORTED and the geometry in the message, the fenced output and frames_after of every stream untouched, and the next
    plain push emits exactly what the twin emits."""
    fft, hop, nm = geo
    s16 = sources(jfk, 3, 3000)
    f32 = [to_f32(x) for x in s16]
    pushes = schedule([len(x) for x in s16], 1000, 14)
    a, b = banks(geo, None, 3, 1000), banks(geo, None, 3, 1000)
    for pcm in (PCM_F32, PCM_S16):
        assert b.bank.supports_io(pcm, OUT_F32) and not b.bank.supports_io(pcm, OUT_F16) and not b.bank.supports_io(pcm, OUT_BF16)
    want = drive(a, f32, pushes, PCM_F32, OUT_F32, plain=True)
    assert sum(int(f.sum()) for f, _ in want) > 20
    same_pushes(drive(b, s16, pushes, PCM_S16, OUT_F32), want, OUT_F32, f"(S16, F32) {geo}")
    x = s16_noise(7, 700)
    fence = DevFence(gpu, 3 * 8 * nm)
    d = gpu.DeviceBuffer(x.nbytes); d.upload(x)
    for pcm, out in [c for c in NEW_COMBOS if c[1] != OUT_F32]:
        before = b.state()
        chunk = x if pcm == PCM_S16 else to_f32(x)
        b.push_host([1], [chunk], pcm, out, expect=ERR_UNSUPPORTED)
        msg = b.lib.melspec_last_error().decode()
        assert re.search(rf"n_fft = {fft}\b", msg) and f"hop = {hop}" in msg and f"n_mels = {nm}" in msg, msg
        b.push_host([0, 2], [], out=out, flush=True, expect=ERR_UNSUPPORTED)
        b.push_device(fence.arm(out), [1], [700 if pcm == PCM_S16 else 350], d.ptr, pcm, out, expect=ERR_UNSUPPORTED)
        assert b.state() == before
    d.free(); fence.buf.free()
    fw, bw = a.push_host([0, 1, 2], [to_f32(x)] * 3, plain=True)
    fg, bg = b.push_host([0, 1, 2], [to_f32(x)] * 3, plain=True)
    assert int(fw.sum()) > 0 and np.array_equal(fg, fw) and np.array_equal(bg, bw)


# ---- 5. detector stage on ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_detector_stage_reads_f32_rows(gpu, banks, jfk):
    """With melspec_stream_enable_vad on, an F16 push and an F16 flush are refused (MELSPEC_ERR_UNSUPPORTED, nothing touched); an
    (S16, F32) push gives the twin's bits and melspec_stream_vad_frames advances as the twin's does."""
    a, b = banks((400, 160, 80), None, 2, 2000), banks((400, 160, 80), None, 2, 2000)
    settings = gpu.DetectionSettings()
    a.bank.enable_vad(settings); b.bank.enable_vad(settings)
    assert b.bank.supports_io(PCM_S16, OUT_F32)
    x = [s16_speech(jfk, 0, 4000), s16_speech(jfk, 1, 4000)]
    emitted = 0
    for lo, hi in ((0, 1777), (1777, 2000), (2000, 4000)):
        before = b.state(), [b.bank.vad_frames(s) for s in (0, 1)]
        b.push_host([0, 1], [c[lo:hi] for c in x], PCM_S16, OUT_F16, expect=ERR_UNSUPPORTED)
        assert "detector" in b.lib.melspec_last_error().decode()
        b.push_host([0, 1], [], out=OUT_F16, flush=True, expect=ERR_UNSUPPORTED)
        assert (b.state(), [b.bank.vad_frames(s) for s in (0, 1)]) == before
        fw, bw = a.push_host([0, 1], [to_f32(c[lo:hi]) for c in x], plain=True)
        fg, bg = b.push_host([0, 1], [c[lo:hi] for c in x], PCM_S16, OUT_F32)
        assert np.array_equal(fg, fw) and np.array_equal(bg, bw)
        assert [b.bank.vad_frames(s) for s in (0, 1)] == [a.bank.vad_frames(s) for s in (0, 1)]
        emitted += int(fg[0])
    assert b.bank.vad_frames(0) == emitted > 20


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_errors_leave_output_and_bank_alone(gpu, banks, jfk):
    """Unknown dtype codes, NULL samples / out / d_out with work to do, a duplicated id: MELSPEC_ERR_INVALID_ARG; a capacity one element
    short, a chunk longer than max_chunk: MELSPEC_ERR_CAPACITY.  After each the output is all sentinel and a valid push gives the twin's
    bits."""
    a, b = banks((400, 160, 80), None, 3, 1000), banks((400, 160, 80), None, 3, 1000)
    x = s16_speech(jfk, 2, 10000)
    pos = [0]
    fence = DevFence(gpu, 3 * 8 * 80)
    d = gpu.DeviceBuffer(2002); d.upload(x[:1001])

    def good(out):
        c = x[pos[0]:pos[0] + 700]; pos[0] += 700
        fw, bw = a.push_host([0, 1, 2], [to_f32(c)] * 3, plain=True)
        fg, bg = b.push_host([0, 1, 2], [c] * 3, PCM_S16, out)
        assert int(fw.sum()) > 0 and np.array_equal(fg, fw) and np.array_equal(bg, round_to(bw, out))

    good(OUT_F16)
    c = x[:700]
    bad = [
        lambda: [b.push_host([0], [c], pcm, out, expect=ERR_INVALID_ARG) for pcm, out in ((2, OUT_F16), (-1, OUT_F32), (PCM_S16, 3), (PCM_S16, -1), (16, OUT_F16))],
        lambda: [b.push_host([0], [], out=out, flush=True, expect=ERR_INVALID_ARG) for out in (3, -1)],
        lambda: [b.push_device(fence.arm(OUT_F16), [0], [700], d.ptr, pcm, out, expect=ERR_INVALID_ARG) for pcm, out in ((2, OUT_F16), (PCM_S16, 3), (-1, -1))],
        lambda: b.push_host([0], [c], PCM_S16, OUT_F16, expect=ERR_INVALID_ARG, null="samples"),
        lambda: b.push_host([0], [c], PCM_S16, OUT_F16, expect=ERR_INVALID_ARG, null="out"),
        lambda: b.push_device(None, [0], [700], d.ptr, PCM_S16, OUT_F16, expect=ERR_INVALID_ARG),
        lambda: b.push_host([0, 1], [c, c], PCM_S16, OUT_F16, expect=ERR_CAPACITY, cap_delta=-1),
        lambda: b.push_host([1], [x[:1001]], PCM_S16, OUT_BF16, expect=ERR_CAPACITY, cap_delta=80),
        lambda: b.push_device(fence.arm(OUT_BF16), [1], [1001], d.ptr, PCM_S16, OUT_BF16, expect=ERR_CAPACITY),
        lambda: b.push_host([2, 2], [c, c], PCM_S16, OUT_F16, expect=ERR_INVALID_ARG),
        lambda: b.push_device(fence.arm(OUT_F16), [2, 0, 2], [160] * 3, d.ptr, PCM_S16, OUT_F16, expect=ERR_INVALID_ARG),
        lambda: b.push_host([3], [c], PCM_S16, OUT_F16, expect=ERR_INVALID_ARG),
    ]
    for k, call in enumerate(bad):
        before = b.state()
        call()
        assert b.state() == before, k
        good((OUT_F16, OUT_BF16, OUT_F32)[k % 3])
    d.free(); fence.buf.free()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_stream_io_symbols_everywhere():
    """the four entry points resolve in the built library and are declared in the header, the ctypes table and the Rust shim"""
    from mel_spec_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "melspec_hip.h")).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    for name in STREAM_IO_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f'"{name}"' in table, name
        assert re.search(rf"\bfn {name}\s*\(", shim), name
    assert lib.melspec_abi_version() == 1


def test_stream_io_null_bank_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.int16)
    ids, lens, frames = np.zeros(1, np.uint32), np.full(1, 512, np.uint32), np.full(1, 0xABCD, np.uint32)
    p, i, ln, fr = _vp(buf), ids.ctypes.data_as(u32p), lens.ctypes.data_as(u32p), frames.ctypes.data_as(u32p)
    for pcm, out in [(PCM_F32, OUT_F32)] + NEW_COMBOS:
        assert lib.melspec_stream_supports_io(None, pcm, out) == 0
        assert lib.melspec_stream_push_host_io(None, i, p, pcm, ln, 1, p, out, 1024, fr) == ERR_INVALID_ARG
        assert b"bank is NULL" in lib.melspec_last_error()
        assert lib.melspec_stream_flush_host_io(None, i, 1, p, out, 1024, fr) == ERR_INVALID_ARG
        assert lib.melspec_stream_push_device_io(None, i, p, pcm, None, ln, 1, p, out, None, fr, None) == ERR_INVALID_ARG
        assert lib.melspec_stream_push_device_io(None, i, None, pcm, None, ln, 1, p, out, None, fr, None) == ERR_INVALID_ARG
    assert frames[0] == 0xABCD and not buf.any()
