"""The centred Whisper features with int16 PCM in and f16 / bf16 out (melspec_whisper_*_io) on the GPU.

The yardsticks are exact, so nothing here is tuned (tests/test_io_dtypes.py has the argument; its generators and sentinels are used):
  * int16 -> f32 is exact, so an int16 call must give THE BITS of the existing f32 call on `s16.astype(float32) * float32(2**-15)`;
  * an f16 / bf16 value is by definition the round-to-nearest-even of the f32 value the existing call writes: numpy's astype(float16) and
    torch's .to(bfloat16) on the CPU are the expected bit patterns -- for the normalised output in both layouts and for the raw rows of
    the split calls, whose d_clip_max stays f32 and is bit-equal to the f32 split call's;
  * rounding is monotone, so the rounded clip maximum equals the largest stored 16-bit value of the clip;
  * against tests/whisper_centered_ref.py the gate is the path's gate (tests/test_whisper_centered.py: F64_TOL 2e-6, F32_TOL 6e-4) plus half
    a unit in the last place of the 16-bit type at the output's magnitude: normalised values of int16-range input lie in [-1.5, 2)
    (2^-11 for f16, 2^-8 for bf16), raw rows in [-10, 4) (4 x the gate, plus 2^-8 / 2^-5).  The ranges are asserted on the reference's own
    values.  In F32 mode the raw rows are compared after folding step 6, as tests/test_whisper_centered.py does: (max(x, g - 8) + 4) / 4
    divides the rows' half-ulp by four.

Every output sits in an allocation filled with the NaN-payload sentinel of its type (f32 0x7FC0DEAD, f16 0x7DAD, bf16 0x7FAD), with a guard
band on each side; every element outside the clips' outputs -- the guard bands, the elements in front of a shifted pointer, the gaps
between caller-chosen offsets -- must keep it.  A 16-bit store at an odd element next to a neighbour's row is exactly where a paired
32-bit store would go wrong.  The samples between the clips of an input buffer are full scale (int16 32767): a frame that read one would
be heard in the bits."""
import ctypes as C

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py); a caller's stream comes from here

import mel_spec_amd as M
import whisper_centered_ref as R
from test_io_dtypes import (ERR_CAPACITY, ERR_INVALID_ARG, ERR_UNSUPPORTED, NEW_COMBOS, OUT_BF16, OUT_F16, OUT_F32, OUT_NP, PCM_F32, PCM_S16, SENTINEL,
                            round_to, s16_extremes, s16_noise, s16_speech, s16_tone, to_f32, to_f64)
from test_whisper_centered import F32_TOL, F64_TOL, MODE_IDS, MODES, PADDED, PLAIN, make

pytestmark = pytest.mark.gpu

GUARD = 64          # guard elements either side of every device output: 128 or 256 bytes, the fenced output keeps its 16-byte alignment
ALL_COMBOS = [(PCM_F32, OUT_F32)] + NEW_COMBOS
HALF_ULP_NORM = {OUT_F32: 0.0, OUT_F16: 2.0 ** -11, OUT_BF16: 2.0 ** -8}        # of values in [1, 2)
HALF_ULP_RAW = {OUT_F32: 0.0, OUT_F16: 2.0 ** -8, OUT_BF16: 2.0 ** -5}          # of values in [8, 16)
SUITE_AND_F32 = (None, "f32")          # None: the mode the suite runs in (AUTO or F64: the f64 kernel); at 128 mels "f32" is the f64 kernel too


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def s16_clip(jfk, clip, n):
    """noise scaled by 2^-k, the speech fixture quantised, a full-scale tone over an -80 dB floor, zeros / +-full scale alternating"""
    if clip % 4 == 3:
        return s16_extremes(clip // 4, n)          # (its own switch is the clip's lowest bit: alternating for 3, 11, ..., zeros for 7, 15, ...)
    return (s16_noise, lambda c, m: s16_speech(jfk, c, m), s16_tone)[clip % 4](clip, n).astype(np.int16)


def s16_clips(jfk, lens, base=0):
    return [s16_clip(jfk, base + i, int(n)) for i, n in enumerate(lens)]


# ---- fenced runs ---------------------------------------------------------------------------------------------------------------------------
class Fence:
    """n elements of the output type `out` between two guard bands, all of it the type's sentinel before the call"""

    def __init__(self, n, out):
        from mel_spec_amd.hip import DeviceBuffer
        self.n, self.dt, self.s = int(n), OUT_NP[out], OUT_NP[out](SENTINEL[out])
        self.es = np.dtype(self.dt).itemsize
        self.buf = DeviceBuffer((self.n + 2 * GUARD) * self.es)
        self.buf.upload(np.full(self.n + 2 * GUARD, self.s, self.dt))
        self.ptr = self.buf.ptr + GUARD * self.es
        assert self.ptr % 16 == 0

    def bits(self):
        a = self.buf.download((self.n + 2 * GUARD,), self.dt)
        assert np.all(a[:GUARD] == self.s) and np.all(a[GUARD + self.n:] == self.s), "guard elements overwritten"
        return a[GUARD:GUARD + self.n]

    def free(self):
        self.buf.free()


def lay_out(clips, pcm, gaps=None):
    """the clips in one buffer of the sample type, gaps[i] (default: 1, 2, 1, ...) full-scale samples in front of clip i and three behind the
    last -> (device buffer, offsets, lengths)"""
    from mel_spec_amd.hip import DeviceBuffer
    dt, loud = (np.int16, 32767) if pcm == PCM_S16 else (np.float32, 1e3)
    gaps = gaps if gaps is not None else [1 + (i & 1) for i in range(len(clips))]
    offs, cur = [], 0
    for g, c in zip(gaps, clips):
        cur += g
        offs.append(cur)
        cur += c.shape[0]
    flat = np.full(cur + 3, loud, dt)
    for o, c in zip(offs, clips):
        flat[o:o + c.shape[0]] = c if pcm == PCM_S16 else to_f32(c)
    d = DeviceBuffer(flat.nbytes)
    d.upload(flat)
    return d, np.array(offs, np.uint64), np.array([c.shape[0] for c in clips], np.uint64)


def place(Ts, n_mels, offsets):
    sizes = [T * n_mels for T in Ts]
    if offsets is None:
        offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if sizes else []
    offsets = [int(o) for o in offsets]
    return offsets, sizes, max([o + n for o, n in zip(offsets, sizes)] + [0])


def collect(bits, offsets, sizes, shift, s):
    used = np.zeros(bits.shape[0], bool)
    for o, n in zip(offsets, sizes):
        assert not used[shift + o:shift + o + n].any(), "the test's own offsets overlap"
        used[shift + o:shift + o + n] = True
    assert np.all(bits[~used] == s), "an element outside the clips' outputs was overwritten"
    parts = [bits[shift + o:shift + o + n].copy() for o, n in zip(offsets, sizes)]
    for i, p in enumerate(parts):
        assert not (p == s).any(), f"clip {i}: {int((p == s).sum())} elements never written"
    return parts


def run(mel, clips, pcm, out, pad_to, split=False, mel_major=True, offsets=None, shift=0, stream=0, plain=False, gaps=None):
    """One ragged call on int16 clips (given to a PCM_F32 call converted) -> (per clip the stored bits, flat in the stored layout; the
    maxima's bits, None for a normalised call).  plain: the existing f32 entry point.  offsets: h_out_offsets / h_rows_offsets in
    elements; shift: the output pointer is advanced by that many elements past the fence's 16-byte aligned start."""
    assert not plain or (pcm, out) == (PCM_F32, OUT_F32)
    d, offs, lens = lay_out(clips, pcm, gaps)
    Ts = [R.num_frames(int(n), pad_to) for n in lens]
    where, sizes, span = place(Ts, mel.n_mels, offsets)
    f = Fence(span + shift, out)
    mx = Fence(len(clips), OUT_F32) if split else None
    ptr, oo = f.ptr + shift * f.es, None if offsets is None else where
    try:
        if split and plain:
            M.whisper_ragged_device_split(mel, d.ptr, offs, lens, ptr, mx.ptr, pad_to, oo, stream)
        elif split:
            M.whisper_ragged_device_split_io(mel, d.ptr, pcm, offs, lens, ptr, out, mx.ptr, pad_to, oo, stream)
        elif plain:
            M.whisper_ragged_device(mel, d.ptr, offs, lens, ptr, pad_to, oo, mel_major, stream)
        else:
            M.whisper_ragged_device_io(mel, d.ptr, pcm, offs, lens, ptr, out, pad_to, oo, mel_major, stream)
        mel.synchronize(stream)
        parts = collect(f.bits(), where, sizes, shift, f.s)
        g = mx.bits().copy() if split else None
    finally:
        d.free(); f.free()
        if mx:
            mx.free()
    return parts, g


_BASE = {}


def base(mel, key, mode, clips, pad_to, split, mel_major=True):
    """the existing f32 call on the converted clips, computed once per session and left unchanged: (per clip the f32 bits, the maxima's bits)"""
    import os
    k = (key, mel.n_mels, mode, os.environ.get("MELSPEC_PRECISE", ""), pad_to, split, mel_major or split)
    if k not in _BASE:
        parts, g = run(mel, clips, PCM_F32, OUT_F32, pad_to, split, mel_major, plain=True)
        for p in parts:
            p.setflags(write=False)
        _BASE[k] = (parts, g)
    return _BASE[k]


def same_bits(got, want32, out, what):
    assert len(got) == len(want32)
    for i, (a, w) in enumerate(zip(got, want32)):
        e = round_to(w, out)
        assert a.shape == e.shape and np.array_equal(a, e), f"{what}: clip {i}: {int((a != e).sum()) if a.shape == e.shape else 'shape'} elements differ from the rounded f32 call"


def check_split(rows, g, want_rows, want_g, out, what):
    """rows = the rounded bits of the f32 split's rows, the maxima bit-equal to the f32 split's, round(g) = the largest stored value"""
    same_bits(rows, want_rows, out, what)
    assert np.array_equal(g, want_g), f"{what}: d_clip_max differs from the f32 split call's"
    for i, r in enumerate(rows):
        if r.size:
            assert to_f64(round_to(g[i:i + 1], out), out)[0] == to_f64(r, out).max(), f"{what}: clip {i}: round(g) is not the largest stored value"
        else:
            assert g[i:i + 1].view(np.float32)[0] == np.float32(-10.0)


def check_all(mel, key, mode, clips, pad_to, what, combos=ALL_COMBOS, **kw):
    """every combination: both layouts and the split call against the f32 calls' bits"""
    for pcm, out in combos:
        for mel_major in (True, False):
            got, _ = run(mel, clips, pcm, out, pad_to, False, mel_major, **kw)
            same_bits(got, base(mel, key, mode, clips, pad_to, False, mel_major)[0], out, f"{what} ({pcm}, {out}) mel_major {mel_major}")
        rows, g = run(mel, clips, pcm, out, pad_to, True, **kw)
        check_split(rows, g, *base(mel, key, mode, clips, pad_to, True), out, f"{what} ({pcm}, {out}) split")


# ---- clip lengths, padding and trimming: each clip alone and all in one ragged batch; (F32, F32) through the _io entry points too -----------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_clip_lengths(jfk, n_mels):
    plain, padded = s16_clips(jfk, PLAIN), s16_clips(jfk, PADDED, base=20)
    for mode in SUITE_AND_F32:
        mel = make(n_mels, mode)
        assert all(M.supports_whisper_io(mel, p, o) for p, o in ALL_COMBOS)
        for n, c in zip(PLAIN, plain):
            check_all(mel, ("len", n), mode, [c], 0, f"n {n} mels {n_mels} mode {mode}", combos=[(PCM_S16, OUT_F16), (PCM_S16, OUT_BF16)])
        for n, c in zip(PADDED, padded):
            check_all(mel, ("pad", n), mode, [c], 4800, f"pad_to 4800 n {n} mels {n_mels} mode {mode}", combos=[(PCM_S16, OUT_F16), (PCM_F32, OUT_BF16)])
        check_all(mel, "len-all", mode, plain, 0, f"all plain lengths, mels {n_mels} mode {mode}")
        check_all(mel, "pad-all", mode, padded, 4800, f"all padded lengths, mels {n_mels} mode {mode}")
        mel.close()


# ---- int16 clips at odd and even samples, outputs at odd and even elements with gaps, in clip order and reversed ---------------------------
def gapped(Ts, n_mels, gaps, order):
    offs, cur = [0] * len(Ts), 0
    for k, i in enumerate(order):
        cur += gaps[k]
        offs[i] = cur
        cur += Ts[i] * n_mels
    return offs


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("pad_to", [0, 10240])
def test_offsets_in_and_out(jfk, pad_to, n_mels):
    lens = [160 * 64, 160 * 128 + 35, 5000, 160 * 72, 1360, 160 * 100 + 7] if pad_to == 0 else [1000, 10040, 0, 5000, 20000, 10239]
    clips = s16_clips(jfk, lens, base=40)
    Ts = [R.num_frames(n, pad_to) for n in lens]
    in_gaps = [1, 2, 2, 1, 3, 1]
    starts = np.cumsum(in_gaps) + np.concatenate([[0], np.cumsum(lens)[:-1]])
    assert any(s & 1 for s in starts) and any(not s & 1 for s in starts), "the int16 clips do not start at odd and at even samples"
    mel = make(n_mels)
    for order in (list(range(6)), list(range(5, -1, -1))):
        offs = gapped(Ts, n_mels, [0, 1, 7, 3, 4, 1], order)
        assert any(o & 1 for o in offs) and any(not o & 1 for o in offs)
        full = [(o & 7) for o, T in zip(offs, Ts) if T % 8 == 0 and T >= 64]
        assert 0 in full and any(full), "the offsets do not turn the 16-byte path both on and off"
        check_all(mel, ("offsets", pad_to), None, clips, pad_to, f"offsets {offs} pad_to {pad_to} mels {n_mels}", combos=NEW_COMBOS, offsets=offs, gaps=in_gaps)
    mel.close()


# ---- the finalise pass's tiles: full and partial last tiles, the 16-byte path on and off by T and by the output pointer ----------------------
TILE_T = [63, 64, 65, 68, 72, 127, 128, 136]
SHIFTS = [0, 1, 2, 4, 8]


def wide(T, off, ptr, es):
    """host::wc_wide_ok, restated: full tiles of this clip leave as 16-byte stores"""
    return ((T | off) & (16 // es - 1)) == 0 and ptr % 16 == 0


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_finalize_tiles(jfk, n_mels, mode, tol):
    clips = s16_clips(jfk, [160 * T for T in TILE_T], base=60)
    mel = make(n_mels, mode)
    # which (T, shift) take the 16-byte path: both on and off for both element sizes; T = 68 on for f32 alone; 72 and 136 on with a partial last tile
    on16 = {(T, s) for T in TILE_T for s in SHIFTS if wide(T, 0, 2 * s, 2)}
    on32 = {(T, s) for T in TILE_T for s in SHIFTS if wide(T, 0, 4 * s, 4)}
    assert on16 == {(T, s) for T in (64, 72, 128, 136) for s in (0, 8)} and on32 == {(T, s) for T in (64, 68, 72, 128, 136) for s in (0, 4, 8)}
    for T, c in zip(TILE_T, clips):
        assert R.frame_classes(c.shape[0], 0) == (T, T - 3, T)
        for shift in SHIFTS:
            for pcm, out in ((PCM_S16, OUT_F16), (PCM_S16, OUT_BF16), (PCM_S16, OUT_F32)):
                got, _ = run(mel, [c], pcm, out, 0, False, True, shift=shift)
                same_bits(got, base(mel, ("tile", T), mode, [c], 0, False, True)[0], out, f"T {T} d_out + {shift} elements ({pcm}, {out})")
        for out in (OUT_F16, OUT_BF16):
            got, _ = run(mel, [c], PCM_S16, out, 0, False, False, shift=1)
            same_bits(got, base(mel, ("tile", T), mode, [c], 0, False, False)[0], out, f"T {T} frame-major d_out + 1 ({out})")
            rows, g = run(mel, [c], PCM_S16, out, 0, True, shift=1)
            check_split(rows, g, *base(mel, ("tile", T), mode, [c], 0, True), out, f"T {T} split d_rows + 1 ({out})")
    check_all(mel, "tile-all", mode, clips, 0, f"T {TILE_T} in one batch, mels {n_mels} mode {mode}", combos=NEW_COMBOS)
    mel.close()


# ---- first_silent inside a tile, on its edge and past it -------------------------------------------------------------------------------------
TILE_PADS = {10240: 64, 11520: 72, 20480: 128}
TILE_PAD_N = [0, 1000, 10040, 10239, 20000]


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_silent_boundary(jfk, n_mels, mode, tol):
    clips = s16_clips(jfk, TILE_PAD_N, base=80)
    mel = make(n_mels, mode)
    for pad_to, T in TILE_PADS.items():
        cls = [R.frame_classes(n, pad_to) for n in TILE_PAD_N]
        assert [c[0] for c in cls] == [T] * len(clips) and [c[2] for c in cls] == [0, 8, 64, min(66, T), min(127, T)], cls
        check_all(mel, ("silent", pad_to), mode, clips, pad_to, f"pad_to {pad_to} mels {n_mels} mode {mode}", combos=NEW_COMBOS)
        for out in (OUT_F16, OUT_BF16):
            rows, g = run(mel, clips, PCM_S16, out, pad_to, True)
            fm, _ = run(mel, clips, PCM_S16, out, pad_to, False, False)
            for i, c in enumerate(cls):
                gi = g[i:i + 1].view(np.float32)[0]
                lo = np.float32(gi - np.float32(8.0))
                silent = np.array([(np.maximum(np.float32(-10.0), lo) + np.float32(4.0)) * np.float32(0.25)], np.float32)
                assert np.all(rows[i].reshape(T, n_mels)[c[2]:] == round_to(np.array([-10.0], np.float32), out)[0]), "a silent frame's raw row is not exactly -10"
                assert np.all(fm[i].reshape(T, n_mels)[c[2]:] == round_to(silent, out)[0]), "a silent frame's normalised row"
        assert to_f64(round_to(np.array([-10.0], np.float32), OUT_BF16), OUT_BF16)[0] == -10.0 == to_f64(round_to(np.array([-10.0], np.float32), OUT_F16), OUT_F16)[0]
    mel.close()


# ---- runs across clips: more than two clips per workgroup, runs that enter a new clip mid-wave --------------------------------------------------
def ragged_1100_s16(oracle):
    from test_whisper_centered import _ragged_1100
    return [s16_noise(i, c.shape[0]) for i, c in enumerate(_ragged_1100(oracle))]          # the same lengths; 2^-(i & 7) per clip


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_ragged_1100(oracle, mode):
    clips = ragged_1100_s16(oracle)
    mel = make(80, mode)
    check_all(mel, "ragged-1100", mode, clips, 0, f"1100 ragged clips, {mode}", combos=[(PCM_S16, OUT_F16)])
    mel.close()


# ---- the uniform calls: a stride past the clip, a stride of zero, trimming, the context's stream and a caller's -----------------------------------
def uniform_io(mel, d_ptr, pcm, out, stride, n, k, pad_to, stream=0):
    T, nm = R.num_frames(n, pad_to), mel.n_mels
    mm, fm, rows, mx = Fence(k * T * nm, out), Fence(k * T * nm, out), Fence(k * T * nm, out), Fence(k, OUT_F32)
    try:
        M.whisper_uniform_device_io(mel, d_ptr, pcm, stride, n, k, mm.ptr, out, pad_to, True, stream)
        M.whisper_uniform_device_io(mel, d_ptr, pcm, stride, n, k, fm.ptr, out, pad_to, False, stream)
        M.whisper_uniform_device_split_io(mel, d_ptr, pcm, stride, n, k, rows.ptr, out, mx.ptr, pad_to, stream)
        mel.synchronize(stream)
        return mm.bits().reshape(k, -1), fm.bits().reshape(k, -1), rows.bits().reshape(k, -1), mx.bits().copy()
    finally:
        mm.free(); fm.free(); rows.free(); mx.free()


def test_uniform_calls_and_streams(jfk):
    from mel_spec_amd.hip import DeviceBuffer
    n, k, stride = 2400, 5, 2400 + 37
    clips = s16_clips(jfk, [n] * k, base=100)
    buf = np.full(stride * k, 32767, np.int16)          # between the clips: not the call's to read
    for i, c in enumerate(clips):
        buf[i * stride:i * stride + n] = c
    d = DeviceBuffer(buf.nbytes)
    d.upload(buf)
    side = torch.cuda.Stream()
    mel = make(80)
    for pad_to, cut in ((0, n), (4800, n), (1600, 1600)):          # 1600: clip_len > pad_to, every clip is trimmed
        want = [c[:cut] for c in clips]
        w_mm, w_fm = (base(mel, ("uniform", pad_to), None, want, pad_to, False, mm)[0] for mm in (True, False))
        w_rows, w_g = base(mel, ("uniform", pad_to), None, want, pad_to, True)
        for out in (OUT_F16, OUT_BF16):
            for stream in (0, side.cuda_stream):
                mm, fm, rows, g = uniform_io(mel, d.ptr, PCM_S16, out, stride, n, k, pad_to, stream)
                same_bits(list(mm), w_mm, out, f"uniform stride {stride} pad_to {pad_to} ({out}) mel-major")
                same_bits(list(fm), w_fm, out, f"uniform stride {stride} pad_to {pad_to} ({out}) frame-major")
                check_split(list(rows), g, w_rows, w_g, out, f"uniform stride {stride} pad_to {pad_to} ({out}) split")
            mm, fm, rows, g = uniform_io(mel, d.ptr, PCM_S16, out, 0, n, 3, pad_to)          # clip_stride == 0: the same clip three times
            same_bits(list(mm), [w_mm[0]] * 3, out, "stride 0 mel-major")
            same_bits(list(fm), [w_fm[0]] * 3, out, "stride 0 frame-major")
            check_split(list(rows), g, [w_rows[0]] * 3, np.repeat(w_g[:1], 3), out, "stride 0 split")
    d.free(); mel.close()


# ---- clips without a frame inside a batch; a batch without any frame ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode", SUITE_AND_F32, ids=["f64", "f32"])
def test_clips_without_a_frame(jfk, mode):
    lens = [1360, 0, 399, 700, 200, 5000]
    clips = s16_clips(jfk, lens, base=120)
    mel = make(80, mode)
    check_all(mel, "frameless", mode, clips, 0, f"lengths {lens}, mode {mode}", combos=NEW_COMBOS)
    none = s16_clips(jfk, [0, 399, 17], base=130)
    for pcm, out in NEW_COMBOS:
        rows, g = run(mel, clips, pcm, out, 0, True)
        assert [r.size for r in rows] == [8 * 80, 0, 0, 4 * 80, 0, 31 * 80] and all(g[i:i + 1].view(np.float32)[0] == np.float32(-10.0) for i in (1, 2, 4))
        d, offs, ln = lay_out(none, pcm)
        f, mx = Fence(64, out), Fence(3, OUT_F32)
        M.whisper_ragged_device_split_io(mel, d.ptr, pcm, offs, ln, f.ptr, out, mx.ptr, 0)
        M.whisper_ragged_device_io(mel, d.ptr, pcm, offs, ln, f.ptr, out, 0)
        mel.synchronize()
        assert np.all(f.bits() == f.s) and np.all(mx.bits().view(np.float32) == np.float32(-10.0)), "a batch without a frame writes g = -10 only"
        d.free(); f.free(); mx.free()
    mel.close()


# ---- stale state: f32 and 16-bit calls of loud and quiet batches on one context against a fresh context -------------------------------------------
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_stale_state(jfk, mode):
    lens = [1360, 5000, 1520, 9000, 700, 400]
    loud = [s16_noise(8 * i, n) for i, n in enumerate(lens)]                 # full scale
    quiet = [(c.astype(np.int32) >> 10).astype(np.int16) for c in loud]      # 60 dB down
    mel, fresh = make(80, mode), make(80, mode)
    want = {}
    for out in (OUT_F16, OUT_BF16):
        want[out] = (run(fresh, quiet, PCM_S16, out, 0, False, True)[0], run(fresh, quiet, PCM_S16, out, 0, True))
    for round_ in range(2):
        for out in (OUT_F16, OUT_BF16):
            run(mel, loud, PCM_F32, OUT_F32, 0, False, True, plain=True)
            run(mel, loud, PCM_S16, out, 0, True)
            run(mel, loud, PCM_F32, OUT_F32, 0, True, plain=True)
            run(mel, loud, PCM_S16, out, 0, False, True)
            rows, g = run(mel, quiet, PCM_S16, out, 0, True)
            norm, _ = run(mel, quiet, PCM_S16, out, 0, False, True)
            assert np.array_equal(g, want[out][1][1]) and all(np.array_equal(a, b) for a, b in zip(rows + norm, want[out][1][0] + want[out][0])), \
                f"a used context differs from a fresh one (out {out}, round {round_})"
        mel.release_scratch()
    mel.close(); fresh.close()


# ---- the host call ---------------------------------------------------------------------------------------------------------------------------------
def test_host_call(jfk):
    from mel_spec_amd import _lib
    x = s16_speech(jfk, 0, jfk.shape[0]).astype(np.int16)
    mel = make(80)
    want = M.whisper_features(mel, to_f32(x))          # the f32 host call: [80][3000], pad_to = 480000
    assert want.shape == (80, 3000)
    for out, name in ((OUT_F16, "f16"), (OUT_BF16, "bf16"), (OUT_F32, "f32")):
        got = M.whisper_features_io(mel, x, out=name)
        assert got.shape == (80, 3000) and got.dtype == np.dtype(M.hip._OUT_NUMPY[out])
        assert np.array_equal(got.view(OUT_NP[out]), round_to(want, out).reshape(80, 3000))
    assert np.array_equal(M.whisper_features_io(mel, to_f32(x), 0, False, "bf16").view(np.uint16), round_to(M.whisper_features(mel, to_f32(x), 0, False), OUT_BF16).reshape(1100, 80))
    # capacity one short: ERR_CAPACITY, the output untouched, *n_frames == 0
    host = np.full(3000 * 80, SENTINEL[OUT_F16], np.uint16)
    nf = C.c_size_t(7)
    rc = _lib.lib().melspec_whisper_compute_host_io(mel._h, x.ctypes.data_as(C.c_void_p), PCM_S16, x.size, 480000, host.ctypes.data_as(C.c_void_p), OUT_F16,
                                                    3000 * 80 - 1, 1, C.byref(nf))
    assert rc == ERR_CAPACITY and nf.value == 0 and np.all(host == SENTINEL[OUT_F16])
    rc = _lib.lib().melspec_whisper_compute_host_io(mel._h, x.ctypes.data_as(C.c_void_p), PCM_S16, x.size, 480000, host.ctypes.data_as(C.c_void_p), OUT_F16,
                                                    3000 * 80, 1, C.byref(nf))
    assert rc == 0 and nf.value == 3000 and np.array_equal(host, round_to(want, OUT_F16).reshape(-1))
    # the batch helpers of the Python frontend
    clips = s16_clips(jfk, [2400, 700, 0, 5000], base=140)
    feats = M.whisper_features_batch(mel, [to_f32(c) for c in clips], 4800)
    rows_w, g_w = M.whisper_split(mel, [to_f32(c) for c in clips], 4800)
    for out, name in ((OUT_F16, "f16"), (OUT_BF16, "bf16")):
        got = M.whisper_features_batch_io(mel, clips, 4800, True, name)
        rows, g = M.whisper_split_io(mel, clips, 4800, name)
        for i in range(len(clips)):
            assert np.array_equal(got[i].view(np.uint16), round_to(feats[i], out).reshape(80, 30)) and np.array_equal(rows[i].view(np.uint16), round_to(rows_w[i], out).reshape(30, 80))
        assert g.dtype == np.float32 and np.array_equal(g, g_w)
    mel.close()


# ---- arguments ---------------------------------------------------------------------------------------------------------------------------------------
def test_arguments(jfk):
    from mel_spec_amd import _lib
    from mel_spec_amd.hip import HipRuntimeError
    L = _lib.lib()
    x = s16_clip(jfk, 1, 4800)

    def code(fn):
        with pytest.raises(HipRuntimeError) as e:
            fn()
        return e.value.code

    for args in ((512, 160, 80), (400, 160, 40), (400, 200, 80)):          # the unsupported contexts
        other = M.HipMelSpectrogram(args[0], args[1], 16000.0, args[2], device=0)
        assert not any(M.supports_whisper_io(other, p, o) for p, o in ALL_COMBOS)
        d, offs, lens = lay_out([x], PCM_S16)
        out, mx = Fence(30 * args[2], OUT_F16), Fence(1, OUT_F32)
        assert code(lambda: M.whisper_ragged_device_io(other, d.ptr, PCM_S16, offs, lens, out.ptr, OUT_F16, 0)) == ERR_UNSUPPORTED
        assert code(lambda: M.whisper_ragged_device_split_io(other, d.ptr, PCM_S16, offs, lens, out.ptr, OUT_F16, mx.ptr, 0)) == ERR_UNSUPPORTED
        assert code(lambda: M.whisper_uniform_device_io(other, d.ptr, PCM_S16, 4800, 4800, 1, out.ptr, OUT_F16, 0)) == ERR_UNSUPPORTED
        assert np.all(out.bits() == out.s) and np.all(mx.bits() == mx.s), "an unsupported context touched its output"
        host = np.full(30 * args[2], SENTINEL[OUT_F16], np.uint16)
        nf = C.c_size_t(7)
        rc = L.melspec_whisper_compute_host_io(other._h, x.ctypes.data_as(C.c_void_p), PCM_S16, x.size, 0, host.ctypes.data_as(C.c_void_p), OUT_F16, host.size, 1, C.byref(nf))
        assert rc == ERR_UNSUPPORTED and nf.value == 0 and np.all(host == SENTINEL[OUT_F16])
        d.free(); out.free(); mx.free(); other.close()
    mel = make(80)
    assert not M.supports_whisper_io(mel, 2, OUT_F16) and not M.supports_whisper_io(mel, PCM_S16, 3) and M.supports_whisper_io(mel, PCM_S16, OUT_BF16)
    d, offs, lens = lay_out([x], PCM_S16)
    out, mx = Fence(30 * 80 + 1, OUT_F16), Fence(1, OUT_F32)
    # unknown dtype codes, on every entry point (the host call included); checked before anything else but the NULL context
    for pcm, o in ((2, OUT_F16), (-1, OUT_F16), (PCM_S16, 3), (PCM_S16, -1)):
        assert code(lambda: M.whisper_ragged_device_io(mel, d.ptr, pcm, offs, lens, out.ptr, o, 1)) == ERR_INVALID_ARG          # (pad_to = 1 is wrong too)
        assert code(lambda: M.whisper_uniform_device_io(mel, d.ptr, pcm, 4800, 4800, 1, out.ptr, o, 0)) == ERR_INVALID_ARG
        assert code(lambda: M.whisper_ragged_device_split_io(mel, d.ptr, pcm, offs, lens, out.ptr, o, mx.ptr, 0)) == ERR_INVALID_ARG
        assert code(lambda: M.whisper_uniform_device_split_io(mel, d.ptr, pcm, 4800, 4800, 1, out.ptr, o, mx.ptr, 0)) == ERR_INVALID_ARG
        nf = C.c_size_t(7)
        host = np.zeros(30 * 80, np.uint16)
        assert L.melspec_whisper_compute_host_io(mel._h, x.ctypes.data_as(C.c_void_p), pcm, x.size, 0, host.ctypes.data_as(C.c_void_p), o, host.size, 1, C.byref(nf)) == ERR_INVALID_ARG
        assert "dtype" in _lib.last_error() and nf.value == 0
    assert L.melspec_whisper_compute_uniform_device_io(None, None, 7, 0, 0, 1, 0, None, 7, 0, None) == ERR_INVALID_ARG and "NULL" in _lib.last_error()
    # an odd byte address for int16 PCM and for a 16-bit output; natural alignment is enough
    assert code(lambda: M.whisper_uniform_device_io(mel, d.ptr + 2 * int(offs[0]) + 1, PCM_S16, 4700, 4700, 1, out.ptr, OUT_F16, 0)) == ERR_INVALID_ARG
    assert "aligned" in _lib.last_error()
    assert code(lambda: M.whisper_uniform_device_io(mel, d.ptr + 2 * int(offs[0]), PCM_S16, 4800, 4800, 1, out.ptr + 1, OUT_BF16, 0)) == ERR_INVALID_ARG
    assert code(lambda: M.whisper_uniform_device_split_io(mel, d.ptr + 2 * int(offs[0]), PCM_S16, 4800, 4800, 1, out.ptr + 1, OUT_F16, mx.ptr, 0)) == ERR_INVALID_ARG
    assert code(lambda: M.whisper_ragged_device_io(mel, d.ptr, PCM_S16, offs, lens, out.ptr + 2, OUT_F32, 0)) == ERR_INVALID_ARG
    for pad in (1, 399):
        assert code(lambda: M.whisper_ragged_device_io(mel, d.ptr, PCM_S16, offs, lens, out.ptr, OUT_F16, pad)) == ERR_INVALID_ARG
        assert code(lambda: M.whisper_uniform_device_split_io(mel, d.ptr, PCM_S16, 4800, 4800, 1, out.ptr, OUT_F16, mx.ptr, pad)) == ERR_INVALID_ARG
        with pytest.raises(HipRuntimeError):
            M.whisper_features_io(mel, x, pad)
    # NULL pointers
    assert code(lambda: M.whisper_uniform_device_split_io(mel, d.ptr, PCM_S16, 4800, 4800, 1, out.ptr, OUT_F16, 0, 0)) == ERR_INVALID_ARG
    assert code(lambda: M.whisper_uniform_device_io(mel, 0, PCM_S16, 4800, 4800, 1, out.ptr, OUT_F16, 0)) == ERR_INVALID_ARG
    assert code(lambda: M.whisper_uniform_device_io(mel, d.ptr, PCM_S16, 4800, 4800, 1, 0, OUT_F16, 0)) == ERR_INVALID_ARG
    assert L.melspec_whisper_compute_ragged_device_io(mel._h, C.c_void_p(d.ptr), PCM_S16, None, None, 1, 0, C.c_void_p(out.ptr), OUT_F16, None, 1, None) == ERR_INVALID_ARG
    mel.synchronize()
    assert np.all(out.bits() == out.s) and np.all(mx.bits() == mx.s)
    # a clip without frames: nothing is written but its maximum
    M.whisper_uniform_device_split_io(mel, d.ptr, PCM_S16, 399, 399, 1, out.ptr, OUT_F16, mx.ptr, 0)
    mel.synchronize()
    assert np.all(out.bits() == out.s) and mx.bits().view(np.float32)[0] == np.float32(-10.0)
    # an odd ELEMENT of a 16-bit output is legal
    M.whisper_uniform_device_io(mel, d.ptr + 2 * int(offs[0]), PCM_S16, 4800, 4800, 1, out.ptr + 2, OUT_F16, 0)
    mel.synchronize()
    b = out.bits()
    assert b[0] == out.s and not (b[1:] == out.s).any()
    d.free(); out.free(); mx.free(); mel.close()


# ---- against the reference ------------------------------------------------------------------------------------------------------------------------------
REF_LENS = [1360, 5000, 700, 9000, 2400, 400, 16000, 3333]
_REF = {}


def reference(jfk, n_mels):
    if n_mels not in _REF:
        clips = s16_clips(jfk, REF_LENS, base=160)
        raws = R.raw_rows_many([to_f32(c) for c in clips], 0, n_mels)
        _REF[n_mels] = (clips, [(raw,) + R.normalise(raw) for raw in raws])
    return _REF[n_mels]


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_against_the_reference(jfk, n_mels, mode, tol):
    clips, want = reference(jfk, n_mels)
    for raw, g, nrm in want:          # the ranges the half-ulp terms rest on
        assert -10.0 <= raw.min() and raw.max() < 4.0 and -1.5 <= nrm.min() and nrm.max() < 2.0
    mel = make(n_mels, mode)
    raw_direct = mode != "f32"
    for pcm, out in NEW_COMBOS:
        norm, _ = run(mel, clips, pcm, out, 0, False, False)
        rows, g = run(mel, clips, pcm, out, 0, True)
        w_n = w_r = w_g = 0.0
        for i, (raw, gw, nrm) in enumerate(want):
            T = raw.shape[0]
            w_n = max(w_n, float(np.abs(to_f64(norm[i], out).reshape(T, n_mels) - nrm).max()))
            gi = float(g[i:i + 1].view(np.float32)[0])
            w_g = max(w_g, abs(gi - gw))
            r = to_f64(rows[i], out).reshape(T, n_mels)
            w_r = max(w_r, float(np.abs(r - raw).max()) if raw_direct else float(np.abs((np.maximum(r, gi - 8.0) + 4.0) / 4.0 - nrm).max()))
        gate_n = tol + HALF_ULP_NORM[out]
        gate_r = 4 * tol + HALF_ULP_RAW[out] if raw_direct else tol + HALF_ULP_RAW[out] / 4
        print(f"({pcm}, {out}) mels {n_mels} mode {mode}: normalised {w_n:.3e} (gate {gate_n:.3e}), g {w_g:.3e}, split {'raw' if raw_direct else 'folded'} {w_r:.3e} (gate {gate_r:.3e})")
        assert w_n <= gate_n, "normalised"
        assert w_g <= 4 * tol, "clip maxima"
        assert w_r <= gate_r, "split rows"
    mel.close()
