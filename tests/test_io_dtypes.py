"""int16 PCM in, f16 / bf16 rows out (melspec_compute_uniform_device_io / _ragged_device_io / _host_io).

The yardsticks are exact, so nothing here is tuned:
  * int16 -> f32 is exact (|v| <= 2^15 fits the 24-bit significand, the scale 2^-15 is a power of two): the int16 call must give THE BITS
    of the existing f32 call on `batch.astype(float32) * float32(2**-15)` (test_conversion_contract pins that statement on the CPU);
  * an f16 / bf16 row is by definition the round-to-nearest-even of the f32 row the existing call writes: numpy's astype(float16) and
    torch's .to(bfloat16) on the CPU are the expected bit patterns;
  * against the oracle the gate is the path's existing gate (tests/test_whole_batch.py: F64 2e-6, AUTO 1e-4, F32 6e-4) plus half a unit in
    the last place of the 16-bit type at the output's magnitude: the rows of int16 input lie in [-1.5, 2), so 2^-11 for f16, 2^-8 for bf16.

Every output is written into the middle of an allocation filled with a sentinel no kernel computes, with a guard band on each side and
-- ragged -- odd element offsets and gaps between the clips:
  f32  0x7FC0DEAD, f16 0x7DAD, bf16 0x7FAD: NaNs with a payload.  The kernels' values are (max(log10(e), ...) + 4) / 4 of finite sums with
  non-negative weights, finite for finite PCM, and a conversion that did produce a NaN would produce the canonical quiet one (0x7E00 /
  0x7FC0), never these payloads.
A 16-bit store at an odd element next to a neighbour's row is exactly where a paired 32-bit store would go wrong."""
import ctypes as C
import os
import re
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT

SR = 16000.0
PCM_F32, PCM_S16 = 0, 1
OUT_F32, OUT_F16, OUT_BF16 = 0, 1, 2
OUT_NP = {OUT_F32: np.uint32, OUT_F16: np.uint16, OUT_BF16: np.uint16}          # bit patterns
SENTINEL = {OUT_F32: 0x7FC0DEAD, OUT_F16: 0x7DAD, OUT_BF16: 0x7FAD}
NEW_COMBOS = [(PCM_S16, OUT_F32), (PCM_F32, OUT_F16), (PCM_F32, OUT_BF16), (PCM_S16, OUT_F16), (PCM_S16, OUT_BF16)]
MODE_TOL = {"f64": 2e-6, "auto": 1e-4, "f32": 6e-4}          # tests/test_whole_batch.py: F64_TOL, TOL, F32_TOL
HALF_ULP = {OUT_F16: 2.0 ** -11, OUT_BF16: 2.0 ** -8}        # of values in [1, 2): the rows of int16 input lie in [-1.5, 2)
GUARD = 4096                                                 # elements of guard band on each side of an output
ERR_INVALID_ARG, ERR_CAPACITY, ERR_UNSUPPORTED = -1, -3, -4
IO_SYMBOLS = ["melspec_supports_io", "melspec_compute_uniform_device_io", "melspec_compute_ragged_device_io", "melspec_compute_host_io"]


# ---- inputs: int16, made on the host from seeds -----------------------------------------------------------------------------------

def s16_noise(clip, n):
    """(a) uniform over the full int16 range, scaled per clip by 2^-k, k = clip & 7"""
    v = np.random.default_rng(1000 + clip).integers(-32768, 32768, n, dtype=np.int32)
    return (v >> (clip & 7)).astype(np.int16)


def s16_speech(jfk, clip, n):
    """(b) the speech fixture scaled to peak 0.9 and rounded to int16 (the fixture's own peak is above 1), rolled per clip, tiled"""
    x = jfk.astype(np.float64) * (0.9 / np.abs(jfk).max())
    q = np.rint(x * 32768.0).astype(np.int16)
    return np.resize(np.roll(q, -2311 * clip), n)


def s16_tone(clip, n):
    """(c) a full-scale tone over a floor 80 dB down: the guard's worst case (tests/test_whole_batch.py: _tone_over_floor)"""
    t = np.arange(n) / SR
    rng = np.random.default_rng(2000 + clip)
    x = 0.999 * np.sin(2 * np.pi * (300.0 + 611.0 * (clip % 11)) * t) + 1e-4 * rng.standard_normal(n)
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def s16_extremes(clip, n):
    """(d) all zeros, and the two extreme values alternating"""
    if clip & 1:
        return np.zeros(n, np.int16)
    return np.where(np.arange(n) & 1, 32767, -32768).astype(np.int16)


def s16_batch(kind, jfk, n_clips, n, base=0):
    make = {"noise": lambda c: s16_noise(c, n), "speech": lambda c: s16_speech(jfk, c, n),
            "mixed": lambda c: (s16_noise, lambda k, m: s16_speech(jfk, k, m), s16_tone, s16_extremes)[c % 4](c, n)}[kind]
    return np.stack([make(base + c) for c in range(n_clips)]) if n_clips else np.zeros((0, n), np.int16)


def to_f32(s16):
    """the conversion contract: exact"""
    return s16.astype(np.float32) * np.float32(2.0 ** -15)


def round_to(out32, out):
    """the expected bit patterns of a 16-bit output from the f32 output (bits in, bits out)"""
    f = np.ascontiguousarray(out32).view(np.float32)
    if out == OUT_F32:
        return f.view(np.uint32)
    if out == OUT_F16:
        return f.astype(np.float16).view(np.uint16)
    return torch.from_numpy(f.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def to_f64(bits, out):
    if out == OUT_F32:
        return bits.view(np.float32).astype(np.float64)
    if out == OUT_F16:
        return bits.view(np.float16).astype(np.float64)
    return (bits.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


# ---- fenced runs ------------------------------------------------------------------------------------------------------------------

class Fence:
    """An output of n elements inside an allocation of n + 2 GUARD elements, all of it the sentinel before the call."""

    def __init__(self, gpu, n, out):
        self.n, self.dt, self.s = int(n), OUT_NP[out], OUT_NP[out](SENTINEL[out])
        self.es = np.dtype(self.dt).itemsize
        self.buf = gpu.DeviceBuffer((self.n + 2 * GUARD) * self.es)
        self.buf.upload(np.full(self.n + 2 * GUARD, self.s, self.dt))
        self.ptr = self.buf.ptr + GUARD * self.es

    def bits(self):
        raw = self.buf.download(self.n + 2 * GUARD, self.dt)
        self.buf.free()
        lo, hi = raw[:GUARD], raw[GUARD + self.n:]
        assert np.all(lo == self.s), f"write below the output: {int(np.sum(lo != self.s))} elements of the lower guard band changed"
        assert np.all(hi == self.s), f"write past the output: {int(np.sum(hi != self.s))} elements of the upper guard band changed"
        return raw[GUARD:GUARD + self.n]


def _upload(gpu, a):
    b = gpu.DeviceBuffer(max(a.nbytes, 16))
    b.upload(np.ascontiguousarray(a))
    return b


def run_uniform(gpu, m, clips, pcm, out, plain=False):
    """clips: [n_clips, n] int16 (PCM_S16) or float32 -> the whole output's bits [n_clips, frames, mels]; plain: the existing f32 call"""
    n_clips, n = clips.shape
    nf, nm = m.num_frames(n), m.n_mels
    d, f = _upload(gpu, clips), Fence(gpu, n_clips * nf * nm, out)
    if plain:
        m.compute_uniform_device(d.ptr, n, n, n_clips, f.ptr)
    else:
        m.compute_uniform_device_io(d.ptr, pcm, n, n, n_clips, f.ptr, out)
    m.synchronize()
    bits = f.bits()
    d.free()
    left = bits == f.s
    assert not left.any(), f"uniform ({pcm}, {out}): {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    return bits.reshape(n_clips, nf, nm)


RAGGED_LENS = [0, 1, 399, 400, 401, 559, 560, 160000, 4321, 0, 720, 16000, 400, 30000, 561, 12345, 0, 1040]


def ragged_tables(m, lens):
    """sample offsets -- a gap of 1 or 2 samples in front of every clip so that at least half of them are odd -- and output offsets in
    elements: odd ones, with gaps between the clips"""
    offs, cur = [], 0
    for c, n in enumerate(lens):
        cur += 1 + (c % 3 == 0)
        offs.append(cur)
        cur += n
    n_samples = cur + 3
    assert sum(o & 1 for o in offs) * 2 >= len(offs)
    frames = [m.num_frames(n) for n in lens]
    oo, cur, gaps = [], 0, []
    for c, f in enumerate(frames):
        g = 1 + 2 * (c % 4)                       # odd gaps: the outputs alternate between odd and even element offsets
        gaps.append((cur, cur + g))
        cur += g
        oo.append(cur)
        cur += f * m.n_mels
    assert any(o & 1 for o, f in zip(oo, frames) if f) and any(not o & 1 for o, f in zip(oo, frames) if f)
    return np.array(offs, np.uint64), n_samples, frames, np.array(oo, np.uint64), cur, gaps


def run_ragged(gpu, m, flat, offs, lens, frames, oo, total, gaps, pcm, out, plain=False):
    """-> per clip [frames, mels] bits; the gaps between the clips must still hold the sentinel"""
    d, f = _upload(gpu, flat), Fence(gpu, total, out)
    if plain:
        m.compute_ragged_device(d.ptr, offs, np.array(lens, np.uint64), f.ptr, oo)
    else:
        m.compute_ragged_device_io(d.ptr, pcm, offs, np.array(lens, np.uint64), f.ptr, out, oo)
    m.synchronize()
    bits = f.bits()
    d.free()
    for a, b in gaps:
        assert np.all(bits[a:b] == f.s), f"ragged ({pcm}, {out}): the gap [{a}, {b}) between two outputs was written"
    res = []
    for c, k in enumerate(frames):
        piece = bits[int(oo[c]):int(oo[c]) + k * m.n_mels]
        assert not (piece == f.s).any(), f"ragged ({pcm}, {out}): clip {c}: {int((piece == f.s).sum())} elements never written"
        res.append(piece.reshape(k, m.n_mels))
    return res


def ragged_flat(kind, jfk, lens, offs, n_samples):
    flat = np.full(n_samples, 12345, np.int16)          # between the clips: samples no frame may read into its result
    for c, (o, n) in enumerate(zip(offs, lens)):
        flat[int(o):int(o) + n] = s16_batch(kind, jfk, 1, n, base=c)[0]
    return flat


def family_of(mode, nm):
    """tests/test_whole_batch.py FAMILIES: the kernel a plain batch of this context runs on"""
    return "six64" if mode == "f64" else ("six16" if nm == 80 else "six12")


def uniform_batch(mode, nm, edge, kind, jfk):
    from test_whole_batch import FAMILIES, _cus, edge_batch, partition
    fam = family_of(mode, nm)
    n_clips, u = edge_batch(fam, edge, _cus())
    fpu = FAMILIES[fam][2]
    frames = u * fpu - (fpu // 2 if u > 1 else 0)          # the clip's last unit partial where it can be
    grid, waves, run, busy = partition(fam, n_clips * u, _cus())
    if edge == "fewer":
        assert n_clips * u < waves or grid < _cus()
    elif edge == "exact":
        assert n_clips * u == waves
    else:
        assert (n_clips * u) % waves == 1 and run >= 2
    return s16_batch(kind, jfk, n_clips, 400 + (frames - 1) * 160)


CASES = [(mode, nm, shape, kind) for mode in ("f64", "f32", "auto") for nm in (80, 128) for shape in ("fewer", "exact", "plus1", "ragged")
         for kind in (("noise", "speech") if mode == "auto" else ("mixed",))]


@pytest.mark.gpu
@pytest.mark.parametrize("mode,nm,shape,kind", CASES, ids=lambda v: str(v))
def test_io_bits_are_the_f32_calls(gpu, jfk, mode, nm, shape, kind):
    """1. int16 in, f32 out == the f32 call on the converted batch, bit for bit (whole output); in AUTO also the same melspec_auto_state
    and the same melspec_guard_count increment -- once on noise (the f32 kernel + recompute tail) and once on speech (the vote hands the
    batch to the f64 kernel).
    2. f32 in, f16 / bf16 out == the round-to-nearest-even of the f32 call's output, bit for bit -- and so is int16 in, f16 / bf16 out.
    Uniform batches at three edges of the run-per-wave partition (fewer units than waves, one unit per wave, several units per wave plus
    one) and a ragged batch with clip lengths 0, 1, 399, 400, 401, 559, 560, 10 s ..., odd sample offsets and odd output offsets."""
    m = gpu.HipMelSpectrogram(400, 160, SR, nm)
    m.set_precision(mode)
    for pcm, out in NEW_COMBOS:
        assert m.supports_io(pcm, out)

    def stats(call):
        before = m.guard_count()
        res = call()
        heavy, frac = m.auto_state()
        return res, (bool(heavy), float(frac), m.guard_count() - before)

    if shape == "ragged":
        offs, n_samples, frames, oo, total, gaps = ragged_tables(m, RAGGED_LENS)
        flat = ragged_flat(kind, jfk, RAGGED_LENS, offs, n_samples)
        run = lambda src, pcm, out, plain=False: run_ragged(gpu, m, src, offs, RAGGED_LENS, frames, oo, total, gaps, pcm, out, plain)
        s16, f32 = flat, to_f32(flat)
        cat = lambda r: np.concatenate([x.reshape(-1) for x in r])
    else:
        s16 = uniform_batch(mode, nm, shape, kind, jfk)
        f32 = to_f32(s16)
        run = lambda src, pcm, out, plain=False: run_uniform(gpu, m, src, pcm, out, plain)
        cat = lambda r: r.reshape(-1)
    want32, st_plain = stats(lambda: cat(run(f32, PCM_F32, OUT_F32, plain=True)))
    if mode == "auto" and shape != "ragged" and shape != "fewer":
        assert st_plain[0] == (kind == "speech"), f"the vote on a {kind} batch: {st_plain}"
    assert np.array_equal(cat(run(f32, PCM_F32, OUT_F32)), want32), "(F32, F32) through the _io call is the plain call"
    for pcm, out in NEW_COMBOS:
        got, st = stats(lambda: cat(run(s16 if pcm == PCM_S16 else f32, pcm, out)))
        want = round_to(want32, out)
        diff = got != want
        assert not diff.any(), f"({pcm}, {out}) {mode} {nm} {shape} {kind}: {int(diff.sum())} of {diff.size} elements differ from the f32 call's " \
                               f"(rounded) bits, first at {int(np.argmax(diff))}: {got[np.argmax(diff)]:#x} != {want[np.argmax(diff)]:#x}"
        if mode == "auto":
            assert st == st_plain, f"({pcm}, {out}): AUTO's statistics (heavy, fraction, guard count) {st} != the f32 call's {st_plain}"
    m.close()


def _oracle_rows(oracle, clips32, nm):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(lambda x: oracle.compute_mel_spectrogram_cpu(x, 400, 160, nm, SR) if x.shape[0] >= 400 else np.zeros((0, nm)), clips32))


def _worst(got_bits, want, out):
    """largest |difference| over every frame of every clip, NaN counting as infinite"""
    worst = 0.0
    for g, w in zip(got_bits, want):
        if w.size:
            d = np.abs(to_f64(g, out) - np.asarray(w, np.float64))
            d[np.isnan(d)] = np.inf
            worst = max(worst, float(d.max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "auto", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
def test_s16_in_16bit_out_against_the_oracle(gpu, oracle, jfk, mode, nm, out):
    """3. int16 in, f16 / bf16 out: every frame of every clip against the oracle on the exactly converted clips.  Gate = the mode's
    existing gate against the oracle (F64 2e-6, AUTO 1e-4, F32 6e-4) + half a unit in the last place of the 16-bit type for rows in
    [-1.5, 2): 2^-11 (f16), 2^-8 (bf16).  A uniform batch of all four input kinds and the ragged batch."""
    m = gpu.HipMelSpectrogram(400, 160, SR, nm)
    m.set_precision(mode)
    gate = MODE_TOL[mode] + HALF_ULP[out]
    clips = s16_batch("mixed", jfk, 12, 400 + 137 * 160)
    got = run_uniform(gpu, m, clips, PCM_S16, out)
    want = _oracle_rows(oracle, list(to_f32(clips)), nm)
    w_uni = _worst(list(got), want, out)
    offs, n_samples, frames, oo, total, gaps = ragged_tables(m, RAGGED_LENS)
    flat = ragged_flat("mixed", jfk, RAGGED_LENS, offs, n_samples)
    got = run_ragged(gpu, m, flat, offs, RAGGED_LENS, frames, oo, total, gaps, PCM_S16, out)
    want = _oracle_rows(oracle, [to_f32(flat[int(o):int(o) + n]) for o, n in zip(offs, RAGGED_LENS)], nm)
    assert [w.shape[0] for w in want] == frames
    lo = min(float(np.min(w)) for w in want if w.size)
    hi = max(float(np.max(w)) for w in want if w.size)
    w_rag = _worst(got, want, out)
    print(f"\nIO-ORACLE {mode} {nm} out={out}: uniform worst {w_uni:.3e}, ragged worst {w_rag:.3e}, gate {gate:.3e}, oracle rows in [{lo:.3f}, {hi:.3f}]")
    assert -1.5 <= lo and hi < 2.0, "the half-ulp term assumes rows in [-1.5, 2)"
    assert w_uni <= gate and w_rag <= gate, (w_uni, w_rag, gate)
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_F32], ids=["f16", "f32"])
def test_host_call_is_the_device_call(gpu, jfk, out):
    """4. melspec_compute_host_io on an int16 clip of 30 s and on one longer than the pipeline's chunk (9 M samples > the 4 Mi samples of a
    chunk, so it is cut; with f32 rows the call is also past the 32 MB of the single-copy path, so the three-stream pipeline runs) equals
    the device call on the same clip bit for bit; short and empty input: zero frames, MELSPEC_OK; one element short: MELSPEC_ERR_CAPACITY."""
    lib = gpu._lib.lib()
    m = gpu.HipMelSpectrogram(400, 160, SR, 80)
    for n in (30 * 16000, 9_000_000):
        x = s16_batch("speech" if n < 10 ** 6 else "noise", jfk, 1, n, base=3)
        host = m.compute_mel_spectrogram(x[0], out_dtype={OUT_F16: "f16", OUT_F32: "f32"}[out])
        assert host.dtype == (np.float16 if out == OUT_F16 else np.float32) and host.shape == (m.num_frames(n), 80)
        dev = run_uniform(gpu, m, x, PCM_S16, out)[0]
        assert np.array_equal(host.view(OUT_NP[out]), dev), f"host call != device call at {n} samples: {int((host.view(OUT_NP[out]) != dev).sum())} elements"
    res = np.full(80 * 4, SENTINEL[out], OUT_NP[out])
    got = C.c_size_t(77)
    short = np.zeros(399, np.int16)
    for k in (399, 0):
        assert lib.melspec_compute_host_io(m._h, short.ctypes.data_as(C.c_void_p), PCM_S16, k, res.ctypes.data_as(C.c_void_p), out, res.size, C.byref(got)) == 0
        assert got.value == 0 and np.all(res == SENTINEL[out])
        got.value = 77
    x = s16_noise(5, 400 + 3 * 160)
    rc = lib.melspec_compute_host_io(m._h, x.ctypes.data_as(C.c_void_p), PCM_S16, x.size, res.ctypes.data_as(C.c_void_p), out, 4 * 80 - 1, C.byref(got))
    assert rc == ERR_CAPACITY and np.all(res == SENTINEL[out])
    assert lib.melspec_compute_host_io(m._h, x.ctypes.data_as(C.c_void_p), PCM_S16, x.size, res.ctypes.data_as(C.c_void_p), out, 4 * 80, C.byref(got)) == 0
    assert got.value == 4 and not np.any(res == SENTINEL[out])
    bf = m.compute_mel_spectrogram(x, out_dtype="bf16")
    assert bf.dtype == np.uint16 and np.array_equal(bf.reshape(-1), round_to(m.compute_mel_spectrogram(to_f32(x)), OUT_BF16).reshape(-1))
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("geo", [(512, 160, 80), (1024, 256, 80)], ids=["512-160-80", "1024-256-80"])
def test_refusals(gpu, geo):
    """5. unknown dtype codes, NULL pointers: MELSPEC_ERR_INVALID_ARG.  A context the feature does not cover: supports_io is 0 for the five
    new combinations and 1 for (F32, F32), the calls return MELSPEC_ERR_UNSUPPORTED with a message that names the geometry, the fenced
    output is untouched, and (F32, F32) through the _io call equals the plain call."""
    lib = gpu._lib.lib()
    fft, hop, nm = geo
    ok = gpu.HipMelSpectrogram(400, 160, SR, 80)
    n = 400 + 20 * 160
    x = s16_noise(1, n)
    d = _upload(gpu, x)
    f = Fence(gpu, 21 * 80, OUT_F16)
    u64p = C.POINTER(C.c_uint64)
    one, ln = np.array([0], np.uint64), np.array([n], np.uint64)
    for pcm, out in ((2, OUT_F16), (-1, OUT_F32), (PCM_S16, 3), (PCM_S16, -1)):
        assert not ok.supports_io(pcm, out)
        assert lib.melspec_compute_uniform_device_io(ok._h, C.c_void_p(d.ptr), pcm, n, n, 1, C.c_void_p(f.ptr), out, None) == ERR_INVALID_ARG
        assert lib.melspec_compute_ragged_device_io(ok._h, C.c_void_p(d.ptr), pcm, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1,
                                                    C.c_void_p(f.ptr), out, None, None) == ERR_INVALID_ARG
        assert lib.melspec_compute_host_io(ok._h, x.ctypes.data_as(C.c_void_p), pcm, n, x.ctypes.data_as(C.c_void_p), out, 10 ** 6, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_uniform_device_io(ok._h, None, PCM_S16, n, n, 1, C.c_void_p(f.ptr), OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_uniform_device_io(ok._h, C.c_void_p(d.ptr), PCM_S16, n, n, 1, None, OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_ragged_device_io(ok._h, C.c_void_p(d.ptr), PCM_S16, None, ln.ctypes.data_as(u64p), 1, C.c_void_p(f.ptr), OUT_F16, None, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_ragged_device_io(ok._h, None, PCM_S16, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1, C.c_void_p(f.ptr), OUT_F16, None, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_host_io(ok._h, None, PCM_S16, n, x.ctypes.data_as(C.c_void_p), OUT_F16, 10 ** 6, None) == ERR_INVALID_ARG
    ok.synchronize()
    ok.close()
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    assert m.supports_io(PCM_F32, OUT_F32)
    n = fft + 20 * hop
    x = s16_noise(2, n)
    d16 = _upload(gpu, x)
    for pcm, out in NEW_COMBOS:
        assert not m.supports_io(pcm, out)
        assert lib.melspec_compute_uniform_device_io(m._h, C.c_void_p(d16.ptr), pcm, n, n, 1, C.c_void_p(f.ptr), out, None) == ERR_UNSUPPORTED
        msg = lib.melspec_last_error().decode()
        assert re.search(rf"n_fft = {fft}\b", msg) and f"hop = {hop}" in msg and f"n_mels = {nm}" in msg, msg
        ln[0] = n
        assert lib.melspec_compute_ragged_device_io(m._h, C.c_void_p(d16.ptr), pcm, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1,
                                                    C.c_void_p(f.ptr), out, None, None) == ERR_UNSUPPORTED
        host_out = np.full(21 * nm, 0x7DAD, np.uint16)
        assert lib.melspec_compute_host_io(m._h, x.ctypes.data_as(C.c_void_p), pcm, n, host_out.ctypes.data_as(C.c_void_p), out, host_out.size, None) == ERR_UNSUPPORTED
        assert np.all(host_out == 0x7DAD)
    m.synchronize()
    assert np.all(f.bits() == np.uint16(SENTINEL[OUT_F16])), "a refused call wrote into the output"
    x32 = to_f32(x)[None, :]
    a = run_uniform(gpu, m, x32, PCM_F32, OUT_F32, plain=True)
    b = run_uniform(gpu, m, x32, PCM_F32, OUT_F32)
    assert np.array_equal(a, b)
    d.free(); d16.free()
    m.close()


@pytest.mark.gpu
def test_config2_at_size_s16_f16(gpu, oracle):
    """6. BASELINE config 2 (1024 x 10 s, 80 mels, default mode) with int16 noise in and f16 rows out: every frame of 64 clips spread over
    the batch against the oracle with the gate of 3 (AUTO 1e-4 + 2^-11), the whole output free of the sentinel."""
    m = gpu.HipMelSpectrogram(400, 160, SR, 80)
    m.set_precision("auto")
    clips = s16_batch("noise", None, 1024, 160000)
    got = run_uniform(gpu, m, clips, PCM_S16, OUT_F16)
    assert not m.auto_state()[0]
    pick = list(range(0, 1024, 16))
    want = _oracle_rows(oracle, [to_f32(clips[c]) for c in pick], 80)
    worst = _worst([got[c] for c in pick], want, OUT_F16)
    gate = MODE_TOL["auto"] + HALF_ULP[OUT_F16]
    print(f"\nIO-AT-SIZE cfg2 (S16, F16): {len(pick)} clips x {got.shape[1]} frames, worst {worst:.3e}, gate {gate:.3e}")
    assert worst <= gate
    m.close()


@pytest.mark.gpu
def test_ctx_entries_share_their_checks(gpu):
    """The f32 entry, the _io entry with (F32, F32) and the _io entry with (S16, F16) of each kind of batch (uniform, ragged, host) run one
    body (ctx_uniform / ctx_ragged / ctx_host): one list of calls walked through the three doors gives one status per call.  The typed door
    alone checks the alignment of the two device pointers -- the f32 entry and (F32, F32) never did, so no misaligned pointer is passed
    through them: such a call would reach a kernel.  Every output is fenced; a refused or empty call leaves every sentinel in place."""
    lib = gpu._lib.lib()
    m = gpu.HipMelSpectrogram(400, 160, SR, 80)
    n, nf, nm = 400 + 20 * 160, 21, 80
    assert m.num_frames(n) == nf and m.num_frames(399) == 0
    x16 = np.stack([s16_noise(1, n), s16_noise(2, n)])
    u64p, f32p = C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    dev = lambda p: None if p is None else C.c_void_p(p)                    # a device address, None = NULL
    tab = lambda a: None if a is None else a.ctypes.data_as(u64p)
    OK = 0

    class Door:
        def __init__(self, name, typed, pcm, out):
            self.name, self.typed, self.pcm, self.out = name, typed, pcm, out
            self.host_in = x16 if pcm == PCM_S16 else to_f32(x16)
            self.src = _upload(gpu, self.host_in)
            self.fence = Fence(gpu, 2 * nf * nm, out)                       # where the refused and the empty calls point
            self.host_out = np.full(nf * nm, SENTINEL[out], OUT_NP[out])

        def uniform(self, pcm_ptr, stride, clip_len, n_clips, out_ptr):
            if not self.typed:
                return lib.melspec_compute_uniform_device(m._h, dev(pcm_ptr), stride, clip_len, n_clips, dev(out_ptr), None)
            return lib.melspec_compute_uniform_device_io(m._h, dev(pcm_ptr), self.pcm, stride, clip_len, n_clips, dev(out_ptr), self.out, None)

        def ragged(self, pcm_ptr, offs, lens, n_clips, out_ptr):
            if not self.typed:
                return lib.melspec_compute_ragged_device(m._h, dev(pcm_ptr), tab(offs), tab(lens), n_clips, dev(out_ptr), None, None)
            return lib.melspec_compute_ragged_device_io(m._h, dev(pcm_ptr), self.pcm, tab(offs), tab(lens), n_clips, dev(out_ptr), self.out, None, None)

        def host(self, samples, n_samples, out, capacity):
            """-> (status, n_frames)"""
            got = C.c_size_t(77)
            if not self.typed:
                rc = lib.melspec_compute_host(m._h, None if samples is None else samples.ctypes.data_as(f32p), n_samples,
                                              None if out is None else out.ctypes.data_as(f32p), capacity, C.byref(got))
            else:
                rc = lib.melspec_compute_host_io(m._h, None if samples is None else samples.ctypes.data_as(C.c_void_p), self.pcm, n_samples,
                                                 None if out is None else out.ctypes.data_as(C.c_void_p), self.out, capacity, C.byref(got))
            return rc, got.value

    doors = [Door("f32 entry", False, PCM_F32, OUT_F32), Door("_io (F32, F32)", True, PCM_F32, OUT_F32), Door("_io (S16, F16)", True, PCM_S16, OUT_F16)]
    zero, one_n, one_399 = np.array([0], np.uint64), np.array([n], np.uint64), np.array([399], np.uint64)
    calls = [
        ("uniform: no clips, NULL pointers", lambda d: d.uniform(None, n, n, 0, None), OK),
        ("uniform: one clip of 399 samples, NULL pointers", lambda d: d.uniform(None, 399, 399, 1, None), OK),
        ("uniform: NULL samples", lambda d: d.uniform(None, n, n, 1, d.fence.ptr), ERR_INVALID_ARG),
        ("uniform: NULL output", lambda d: d.uniform(d.src.ptr, n, n, 1, None), ERR_INVALID_ARG),
        ("uniform: two clips, clip_stride = clip_len - 1", lambda d: d.uniform(d.src.ptr, n - 1, n, 2, d.fence.ptr), ERR_INVALID_ARG),
        ("ragged: no clips, NULL pointers", lambda d: d.ragged(None, None, None, 0, None), OK),
        ("ragged: one clip of 399 samples, NULL device pointers", lambda d: d.ragged(None, zero, one_399, 1, None), OK),
        ("ragged: NULL samples", lambda d: d.ragged(None, zero, one_n, 1, d.fence.ptr), ERR_INVALID_ARG),
        ("ragged: NULL output", lambda d: d.ragged(d.src.ptr, zero, one_n, 1, None), ERR_INVALID_ARG),
        ("ragged: NULL offsets", lambda d: d.ragged(d.src.ptr, None, one_n, 1, d.fence.ptr), ERR_INVALID_ARG),
        ("ragged: NULL lengths", lambda d: d.ragged(d.src.ptr, zero, None, 1, d.fence.ptr), ERR_INVALID_ARG),
        ("host: 399 samples, NULL pointers", lambda d: d.host(None, 399, None, 0), (OK, 0)),
        ("host: NULL samples", lambda d: d.host(None, n, d.host_out, d.host_out.size), (ERR_INVALID_ARG, 0)),
        ("host: NULL output", lambda d: d.host(d.host_in[0], n, None, nf * nm), (ERR_INVALID_ARG, 0)),
        ("host: capacity one element short", lambda d: d.host(d.host_in[0], n, d.host_out, nf * nm - 1), (ERR_CAPACITY, 0)),
    ]
    for what, call, want in calls:
        got = [call(d) for d in doors]
        assert got == [want] * 3, f"{what}: {dict(zip((d.name for d in doors), got))}, expected {want} from every door"
    typed = doors[2]
    for what, got in (("uniform: samples at an odd byte address", typed.uniform(typed.src.ptr + 1, n, n, 1, typed.fence.ptr)),
                      ("uniform: rows at an odd byte address", typed.uniform(typed.src.ptr, n, n, 1, typed.fence.ptr + 1)),
                      ("ragged: samples at an odd byte address", typed.ragged(typed.src.ptr + 1, zero, one_n, 1, typed.fence.ptr)),
                      ("ragged: rows at an odd byte address", typed.ragged(typed.src.ptr, zero, one_n, 1, typed.fence.ptr + 1))):
        assert got == ERR_INVALID_ARG, f"{what} through {typed.name}: {got}"
    m.synchronize()
    for d in doors:
        assert np.all(d.host_out == SENTINEL[d.out]), f"{d.name}: a refused host call wrote into the output"
        assert np.all(d.fence.bits() == d.fence.s), f"{d.name}: a refused or empty call wrote into the output"
    # two clips with clip_stride = 0: every clip is the first one -- accepted by every door, and both outputs are clip 0's rows
    rows = []
    for d in doors:
        f = Fence(gpu, 2 * nf * nm, d.out)
        assert d.uniform(d.src.ptr, 0, n, 2, f.ptr) == OK, d.name
        m.synchronize()
        bits = f.bits().reshape(2, nf * nm)
        assert not np.any(bits == f.s) and np.array_equal(bits[0], bits[1]), d.name
        rows.append(bits)
        d.src.free()
    assert np.array_equal(rows[0], rows[1])
    m.close()


@pytest.mark.gpu
def test_f32_through_io_is_the_plain_call_ragged_and_host(gpu):
    """(F32, F32) through melspec_compute_ragged_device_io / melspec_compute_host_io gives the bits of melspec_compute_ragged_device /
    melspec_compute_host: three clips of 399, 400 and 400 + 7 * 160 + 1 samples (no frame, one frame, a tail of one sample behind the last
    frame), packed and at output offsets that leave gaps; the host pair on the third clip.  (test_refusals compares the uniform pair.)"""
    lib = gpu._lib.lib()
    m = gpu.HipMelSpectrogram(400, 160, SR, 80)
    lens = [399, 400, 400 + 7 * 160 + 1]
    frames = [m.num_frames(k) for k in lens]
    assert frames == [0, 1, 8]
    clips = [to_f32(s16_noise(20 + c, k)) for c, k in enumerate(lens)]
    offs = np.array([0, 399, 799], np.uint64)
    d = _upload(gpu, np.concatenate(clips))
    for oo in (None, np.array([3, 8, 8 + 80 + 5], np.uint64)):
        total = 9 * 80 if oo is None else int(oo[2]) + 8 * 80 + 7
        got = []
        for plain in (True, False):
            f = Fence(gpu, total, OUT_F32)
            if plain:
                m.compute_ragged_device(d.ptr, offs, lens, f.ptr, oo)
            else:
                m.compute_ragged_device_io(d.ptr, PCM_F32, offs, lens, f.ptr, OUT_F32, oo)
            m.synchronize()
            got.append(f.bits())
            assert int(np.sum(got[-1] != f.s)) == 9 * 80, "nine frames are written, and nothing between them"
        assert np.array_equal(got[0], got[1]), "ragged (F32, F32) through the _io call is the plain call"
    d.free()
    x = clips[2]
    a = m.compute_mel_spectrogram(x)                                         # melspec_compute_host
    b = np.full((8, 80), SENTINEL[OUT_F32], np.uint32)
    n_frames = C.c_size_t(0)
    assert lib.melspec_compute_host_io(m._h, x.ctypes.data_as(C.c_void_p), PCM_F32, x.size, b.ctypes.data_as(C.c_void_p), OUT_F32, b.size, C.byref(n_frames)) == 0
    assert n_frames.value == 8 and a.shape == (8, 80)
    assert np.array_equal(a.view(np.uint32), b), "host (F32, F32) through the _io call is the plain call"
    m.close()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_io_symbols_everywhere():
    """the four entry points resolve in the built library and are declared in the header, the ctypes table and the Rust shim"""
    from mel_spec_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "melspec_hip.h")).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    for name in IO_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f'"{name}"' in table, name
        assert re.search(rf"\bfn {name}\s*\(", shim), name
    for macro, value in (("MELSPEC_PCM_F32", 0), ("MELSPEC_PCM_S16", 1), ("MELSPEC_OUT_F32", 0), ("MELSPEC_OUT_F16", 1), ("MELSPEC_OUT_BF16", 2)):
        assert re.search(rf"#define\s+{macro}\s+{value}\b", header), macro
    assert lib.melspec_abi_version() == 1


def test_io_null_context_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.int16)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.melspec_supports_io(None, PCM_S16, OUT_F16) == 0
    assert lib.melspec_compute_uniform_device_io(None, p, PCM_S16, 1024, 1024, 1, p, OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_ragged_device_io(None, p, PCM_S16, None, None, 1, p, OUT_F16, None, None) == ERR_INVALID_ARG
    assert lib.melspec_compute_host_io(None, p, PCM_S16, 1024, p, OUT_F16, 1024, None) == ERR_INVALID_ARG
    assert b"ctx is NULL" in lib.melspec_last_error()


def test_conversion_contract():
    """The yardstick of the GPU tests: for all 65 536 int16 values float32(v) * float32(2^-15) is exactly v / 32768 -- no rounding in the
    conversion, none in the scale -- and equals the reference's `v as f32 / 32768.0`."""
    v = np.arange(-32768, 32768, dtype=np.int64)
    f = v.astype(np.int16).astype(np.float32) * np.float32(2.0 ** -15)
    assert f.dtype == np.float32
    assert np.array_equal(f.astype(np.float64), v / 32768.0)                        # exactly representable
    assert np.array_equal(f, (v / 32768.0).astype(np.float32))
    assert np.array_equal(f, v.astype(np.float32) / np.float32(32768.0))            # the reference's spelling
    assert np.array_equal(to_f32(v.astype(np.int16)), f)
    # and the 16-bit sentinels are NaNs with a payload, not the canonical quiet NaN a conversion produces
    assert np.isnan(np.array([0x7DAD], np.uint16).view(np.float16)[0]) and 0x7DAD != 0x7E00
    assert np.isnan((np.array([0x7FAD], np.uint32) << 16).view(np.float32)[0]) and 0x7FAD != 0x7FC0
