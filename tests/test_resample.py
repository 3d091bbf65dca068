"""The polyphase resampler on the GPU (melspec_resample_*, include/melspec_resample.h) against the numpy f64 model of its definition
(tests/resample_ref.py), at every output:
    |y_gpu - y_ref| <= 1/2 spacing_f32(y_ref) + n_inside 2^-52 A + 2^-49 X + 2^-126,   A = sum |h_k x_k|, X = sum |x_k| over the inside taps
(one rounding to f32; the f64 summation bound in any order, fused or not; the tap table's 2^-49 allowance; a flushed subnormal).
Clips of a few hundred to a few thousand samples around every edge of the definition and of the kernel's tiles; every clip sits in a
sentinel-filled output, between samples that must not be read (NaN / full scale).  The bit equalities: (S16) == (F32) on the converted
batch, uniform == ragged == host, independence of neighbours, position, out_offsets, strides and an odd int16 start, the shift by orig,
a repeated call, the copy at rate_in == rate_out.  A grid of 1100 clips, one +Inf sample, the stream order in front of the Whisper call,
and every status of the header with an untouched output."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch          # before libmelspec_hip.so is loaded: the caller's streams

import resample_ref as R

pytestmark = pytest.mark.gpu

RATES = [(48000, 16000), (44100, 16000), (8000, 16000), (32000, 16000), (22050, 16000), (24000, 16000), (16000, 24000)]
IDS = [f"{a}-{b}" for a, b in RATES]
SENTINEL = np.float32(-7777.25)
S16, F32 = "s16", "f32"


def tile_samples(rate_in, rate_out):
    """input samples whose outputs fill one tile of the kernel (mel_spec_amd/csrc/resample_plan.hpp: rs_launch)"""
    orig, new, width, K, _, _ = R.geometry(rate_in, rate_out)
    taps = int(R.inside(rate_in, rate_out).sum(axis=1).max())
    tab = taps * new * 8 + new * 4 + 8
    blocks = max(1, 1024 // new)
    span = lambda b: (b * orig + 2 * width) * 8
    room = 65536 - tab if tab + span(1) <= 65536 else 65536
    while blocks > 1 and span(blocks) > room:
        blocks -= 1
    return blocks * orig


def edge_lengths(rate_in, rate_out):
    orig, new, width, K, _, _ = R.geometry(rate_in, rate_out)
    t = tile_samples(rate_in, rate_out)
    return sorted({0, 1, 2, max(orig - 1, 0), orig, orig + 1, width, K - 1, K, K + 1, t - 1, t, t + 1, 3 * t + 2 * (orig // 2) + 1})


@functools.lru_cache(maxsize=None)
def clip(seed, n):
    """a seeded normal x 0.3: (f32, int16) -- two clips of their own, the int16 one clipped to full scale"""
    x = np.random.default_rng(seed).standard_normal(n) * 0.3
    f = x.astype(np.float32)
    s = np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)
    f.setflags(write=False); s.setflags(write=False)
    return f, s


@functools.lru_cache(maxsize=None)
def model(rate_in, rate_out, seed, n, dtype):
    """(y f64, tolerance) of clip(seed, n): computed once, shared, left unchanged"""
    x = clip(seed, n)[dtype == S16]
    y, A, X, n_in = R.resample(x, rate_in, rate_out, bounds=True)
    tol = R.tolerance(y, A, X, n_in)
    y.setflags(write=False); tol.setflags(write=False)
    return y, tol


def lay_out(clips, dtype, gaps, lead=0):
    """the clips in one buffer, gaps[i] samples that must not be read in front of clip i (f32: NaN, int16: full scale) and one behind
    the last; `lead`: samples in front of everything (an odd one makes every int16 address odd when the gaps are even)"""
    np_t = np.int16 if dtype == S16 else np.float32
    bad = np.int16(32767) if dtype == S16 else np.float32(np.nan)
    parts, offs, pos = [np.full(lead, bad, np_t)], [], lead
    for c, g in zip(clips, gaps):
        parts.append(np.full(g, bad, np_t)); pos += g
        offs.append(pos)
        parts.append(np.asarray(c, np_t)); pos += len(c)
    parts.append(np.full(8, bad, np_t))
    return np.concatenate(parts), np.array(offs, np.uint64), np.array([len(c) for c in clips], np.uint64)


class Dev:
    """device buffers that are freed with the test"""

    def __init__(self, gpu):
        self.gpu, self.bufs = gpu, []

    def put(self, a):
        b = self.gpu.DeviceBuffer(max(a.nbytes, 16))
        b.upload(a)
        self.bufs.append(b)
        return b

    def sentinel(self, n):
        return self.put(np.full(max(n, 4), SENTINEL, np.float32))

    def free(self):
        for b in self.bufs:
            b.free()


def ragged(gpu, rs, clips, dtype, gaps=None, out_gaps=None, lead=0, stream=None):
    """the clips through the ragged call: their outputs, after checking that nothing outside them changed"""
    d = Dev(gpu)
    try:
        gaps = gaps if gaps is not None else [2 * (i % 3) for i in range(len(clips))]
        flat, offs, lens = lay_out(clips, dtype, gaps, lead)
        n_out = [rs.out_len(len(c)) for c in clips]
        out_gaps = out_gaps if out_gaps is not None else [1 + i % 4 for i in range(len(clips))]
        oo = np.cumsum([g + (n_out[i - 1] if i else 0) for i, g in enumerate(out_gaps)]).astype(np.uint64)
        total = int(oo[-1]) + n_out[-1] + 5
        d_in, d_out = d.put(flat), d.sentinel(total)
        rs.compute_ragged_device(d_in.ptr, dtype, offs, lens, d_out.ptr, oo, stream)
        rs.synchronize(stream)
        got = d_out.download((total,))
        mask = np.ones(total, bool)
        res = []
        for o, n in zip(oo, n_out):
            mask[int(o):int(o) + n] = False
            res.append(got[int(o):int(o) + n].copy())
        assert np.all(got[mask] == SENTINEL), "a store outside [0, out_len) of a clip"
        return res
    finally:
        d.free()


def uniform(gpu, rs, clips, dtype, pad_in=3, pad_out=2):
    d = Dev(gpu)
    try:
        n = len(clips[0])
        assert all(len(c) == n for c in clips)
        np_t = np.int16 if dtype == S16 else np.float32
        bad = np.int16(32767) if dtype == S16 else np.float32(np.nan)
        stride, n_out = n + pad_in, rs.out_len(n)
        ostride = n_out + pad_out
        flat = np.full(stride * len(clips) + 8, bad, np_t)
        for i, c in enumerate(clips):
            flat[i * stride:i * stride + n] = c
        d_in, d_out = d.put(flat), d.sentinel(ostride * len(clips) + 8)
        rs.compute_uniform_device(d_in.ptr, dtype, stride, n, len(clips), d_out.ptr, ostride)
        rs.synchronize()
        got = d_out.download((ostride * len(clips) + 8,))
        res = [got[i * ostride:i * ostride + n_out].copy() for i in range(len(clips))]
        for i in range(len(clips)):
            got[i * ostride:i * ostride + n_out] = SENTINEL
        assert np.all(got == SENTINEL), "a store outside [0, out_len) of a clip"
        return res
    finally:
        d.free()


def same_bits(a, b, what=""):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), f"{what}: {int((a.view(np.uint32) != b.view(np.uint32)).sum())} of {a.size} values differ"


def within(got, rate_in, rate_out, seed, n, dtype, what=""):
    y, tol = model(rate_in, rate_out, seed, n, dtype)
    assert got.shape == y.shape, (what, got.shape, y.shape)
    if y.size:
        err = np.abs(got.astype(np.float64) - y)
        worst = int(np.argmax(err - tol))
        assert np.all(err <= tol), f"{what} n={n}: output {worst}: |{got[worst]!r} - {y[worst]!r}| = {err[worst]:.3e} > {tol[worst]:.3e}"


# ---- values at every edge; S16 == F32 on the converted batch; uniform == ragged == host ----
@pytest.mark.parametrize("pair", RATES, ids=IDS)
def test_values_and_edges(gpu, pair):
    rs = gpu.Resampler(*pair)
    assert rs.kernel_name == "resample_kernel<lds samples, lds taps>"
    lens = edge_lengths(*pair)
    for dtype in (S16, F32):
        clips = [clip(100 + i, n)[dtype == S16] for i, n in enumerate(lens)]
        outs = ragged(gpu, rs, clips, dtype)
        for i, (n, got) in enumerate(zip(lens, outs)):
            assert got.size == R.out_len(*pair, n) == rs.out_len(n)
            within(got, *pair, 100 + i, n, dtype, f"{pair} {dtype}")
        if dtype == S16:
            conv = [c.astype(np.float32) / np.float32(32768.0) for c in clips]
            for a, b in zip(outs, ragged(gpu, rs, conv, F32)):
                same_bits(a, b, "(S16) against (F32) on v / 32768")
        for i, n in enumerate(lens):
            if n in (lens[3], lens[-1], lens[-3]):
                u = uniform(gpu, rs, [clips[i], clips[i][::-1].copy(), clips[i]], dtype)
                same_bits(u[0], outs[i], "uniform against ragged")
                same_bits(u[2], outs[i], "the third clip of a uniform batch against the first")
            same_bits(rs.compute(clips[i]), outs[i], f"host against ragged, n={n}")
    rs.close()


# ---- a clip's output depends on the clip alone ----
@pytest.mark.parametrize("pair", [RATES[0], RATES[1], RATES[2], RATES[6]], ids=[IDS[0], IDS[1], IDS[2], IDS[6]])
def test_independence_shift_and_repeat(gpu, pair):
    rs = gpu.Resampler(*pair)
    orig, new = R.geometry(*pair)[:2]
    t = tile_samples(*pair)
    lens = [t + 37, 5, 0, 2 * t + 1, 333]
    for dtype in (S16, F32):
        clips = [clip(200 + i, n)[dtype == S16] for i, n in enumerate(lens)]
        base = ragged(gpu, rs, clips, dtype)
        again = ragged(gpu, rs, clips, dtype)
        perm = [3, 0, 4, 2, 1]
        moved = ragged(gpu, rs, [clips[i] for i in perm], dtype, gaps=[1, 7, 0, 3, 5], out_gaps=[9, 0, 3, 0, 40], lead=1)      # odd int16 starts among them
        odd = ragged(gpu, rs, clips, dtype, gaps=[0, 2, 4, 6, 8], lead=1)                                                      # every int16 start odd
        for i in range(len(clips)):
            same_bits(again[i], base[i], "a second identical call")
            same_bits(moved[perm.index(i)], base[i], "another position, other neighbours, other out_offsets")
            same_bits(odd[i], base[i], "an odd start")
            within(base[i], *pair, 200 + i, lens[i], dtype, f"{pair} {dtype}")
        np_t = clips[0].dtype
        shifted = ragged(gpu, rs, [np.concatenate([np.zeros(orig, np_t), c]) for c in clips], dtype)
        for i in range(len(clips)):
            assert shifted[i].size == base[i].size + new
            same_bits(shifted[i][new:], base[i], "orig leading zeros shift the output by new")
    rs.close()


def test_equal_rates_copy(gpu):
    rs = gpu.Resampler(16000, 16000)
    assert rs.kernel_name == "resample_kernel<copy>"
    lens = [0, 1, 1023, 1024, 1025, 3 * 1024 + 77]
    for dtype in (S16, F32):
        clips = [clip(300 + i, n)[dtype == S16] for i, n in enumerate(lens)]
        outs = ragged(gpu, rs, clips, dtype, lead=1)
        for c, got in zip(clips, outs):
            want = c.astype(np.float32) / np.float32(32768.0) if dtype == S16 else c
            same_bits(got, want, "rate_in == rate_out is the converted input")
            same_bits(rs.compute(c), want, "host")
        same_bits(uniform(gpu, rs, [clips[-1], clips[-1]], dtype)[1], outs[-1], "uniform")
    rs.close()


# ---- the forms of the kernel off the usual rates: taps in their global table; samples read from the clip ----
@pytest.mark.parametrize("pair,name", [((11025, 16000), "resample_kernel<lds samples, global taps>"), ((4000, 1), "resample_kernel<global samples, global taps>")],
                         ids=["11025-16000", "4000-1"])
def test_other_forms(gpu, pair, name):
    rs = gpu.Resampler(*pair)
    assert rs.kernel_name == name
    orig, new, width, K, _, _ = R.geometry(*pair)
    lens = [0, 1, orig + 1, 2 * orig + 3, 3 * orig + 500] if new > 1 else [0, 1, orig, orig + 1, 5 * orig + 3]
    for dtype in (S16, F32):
        clips = [clip(400 + i, n)[dtype == S16] for i, n in enumerate(lens)]
        outs = ragged(gpu, rs, clips, dtype, lead=1)
        for i, (n, got) in enumerate(zip(lens, outs)):
            within(got, *pair, 400 + i, n, dtype, f"{pair} {dtype}")
            same_bits(rs.compute(clips[i]), got, "host against ragged")
    rs.close()


# ---- more workgroups than CUs: 1100 ragged clips of 0-3 tiles in one call ----
def test_grid(gpu):
    pair = (48000, 16000)
    rs = gpu.Resampler(*pair)
    t = tile_samples(*pair)
    lens = np.random.default_rng(77).integers(0, 3 * t + 1, 1100)
    lens[:6] = [0, t, 3 * t, 1, t + 1, 0]
    clips = [clip(500 + i % 7, int(n))[1] for i, n in enumerate(lens)]
    outs = ragged(gpu, rs, clips, S16, lead=1)
    assert sum(-(-rs.out_len(int(n)) // 1024) for n in lens) > 1500
    for i, (n, got) in enumerate(zip(lens, outs)):
        within(got, *pair, 500 + i % 7, int(n), S16, f"clip {i}")
    rs.close()


# ---- one +Inf sample ----
@pytest.mark.parametrize("pair", [RATES[0], RATES[1], RATES[2]], ids=IDS[:3])
def test_one_infinite_sample(gpu, pair):
    rs = gpu.Resampler(*pair)
    orig, new, width, K, _, _ = R.geometry(*pair)
    ins = R.inside(*pair)
    n = tile_samples(*pair) + 4 * K + 11
    x = clip(600, n)[0].copy()
    clean = ragged(gpu, rs, [x], F32)[0]
    at = n // 2
    x[at] = np.inf
    got = ragged(gpu, rs, [x], F32)[0]
    i = np.arange(got.size)
    j, p = i // new, i % new
    k = at - j * orig + width                              # the tap that meets the sample
    in_dense = (k >= 0) & (k < K)
    in_inside = in_dense & ins[p, np.clip(k, 0, K - 1)]
    assert in_inside.sum() >= 10 and (~in_dense).sum() >= got.size // 2
    same_bits(got[~in_dense], clean[~in_dense], "outputs whose dense window excludes the sample")
    assert not np.any(np.isfinite(got[in_inside])), "outputs whose inside taps include the sample are non-finite"
    rs.close()


# ---- stream order: the resampler's output feeds the Whisper call on the same stream, no synchronise between ----
def test_stream_order_in_front_of_whisper(gpu):
    rs = gpu.Resampler(48000, 16000)
    mel = gpu.HipMelSpectrogram(400, 160, 16000.0, 80, device=0)
    assert gpu.supports_whisper(mel)
    n_clips, n_in = 3, 48000
    n = rs.out_len(n_in)
    T = gpu.whisper_num_frames(mel, n, 0)
    assert n == 16000 and T == 100
    d = Dev(gpu)
    side = torch.cuda.Stream()
    st = side.cuda_stream
    try:
        pcm = np.concatenate([clip(700 + i, n_in)[1] for i in range(n_clips)])
        d_in, d_mid, d_feat, d_feat2 = d.put(pcm), d.sentinel(n_clips * n), d.sentinel(n_clips * T * 80), d.sentinel(n_clips * T * 80)
        rs.compute_uniform_device(d_in.ptr, S16, n_in, n_in, n_clips, d_mid.ptr, n, st)
        gpu.whisper_uniform_device(mel, d_mid.ptr, n, n, n_clips, d_feat.ptr, 0, True, st)
        mel.synchronize(st)
        mid = d_mid.download((n_clips * n,))
        feat = d_feat.download((n_clips * T * 80,))
        assert not np.any(mid == SENTINEL)
        d_copy = d.put(mid)
        gpu.whisper_uniform_device(mel, d_copy.ptr, n, n, n_clips, d_feat2.ptr, 0, True, st)
        mel.synchronize(st)
        same_bits(feat, d_feat2.download((n_clips * T * 80,)), "the Whisper call behind the resampler against the call on a copy of its output")
        assert np.all(np.isfinite(feat)) and not np.any(feat == SENTINEL)
    finally:
        d.free()
        mel.close()
        rs.close()


# ---- every status of the header; a refused call leaves its output untouched ----
def test_statuses(gpu):
    from mel_spec_amd import _lib
    L = _lib.lib()
    rs = gpu.Resampler(48000, 16000)
    h = rs._h
    d = Dev(gpu)
    try:
        x = clip(800, 3000)[1]
        d_in, d_out = d.put(x), d.sentinel(1200)
        pin, pout = d_in.ptr, d_out.ptr
        vp = C.c_void_p
        offs = np.array([0, 1000], np.uint64); lens = np.array([1000, 2000], np.uint64)
        po, pl = offs.ctypes.data_as(C.POINTER(C.c_uint64)), lens.ctypes.data_as(C.POINTER(C.c_uint64))
        INV = _lib.ERR_INVALID_ARG
        refused = [
            ("NULL handle", INV, lambda: L.melspec_resample_uniform_device(None, vp(pin), 1, 1500, 1500, 2, vp(pout), 500, None)),
            ("NULL handle before the dtype", INV, lambda: L.melspec_resample_ragged_device(None, vp(pin), 9, po, pl, 2, vp(pout), None, None)),
            ("dtype", INV, lambda: L.melspec_resample_uniform_device(h, vp(pin), 2, 1500, 1500, 2, vp(pout), 500, None)),
            ("dtype before NULL pointers", INV, lambda: L.melspec_resample_ragged_device(h, None, -1, po, pl, 2, None, None, None)),
            ("NULL d_pcm", INV, lambda: L.melspec_resample_uniform_device(h, None, 1, 1500, 1500, 2, vp(pout), 500, None)),
            ("NULL d_out", INV, lambda: L.melspec_resample_uniform_device(h, vp(pin), 1, 1500, 1500, 2, None, 500, None)),
            ("NULL offsets", INV, lambda: L.melspec_resample_ragged_device(h, vp(pin), 1, None, pl, 2, vp(pout), None, None)),
            ("NULL lengths", INV, lambda: L.melspec_resample_ragged_device(h, vp(pin), 1, po, None, 2, vp(pout), None, None)),
            ("NULL before misaligned", INV, lambda: L.melspec_resample_ragged_device(h, None, 1, po, pl, 2, vp(pout + 2), None, None)),
            ("odd int16 address", INV, lambda: L.melspec_resample_uniform_device(h, vp(pin + 1), 1, 1400, 1400, 2, vp(pout), 500, None)),
            ("f32 samples at 2 mod 4", INV, lambda: L.melspec_resample_uniform_device(h, vp(pin + 2), 0, 700, 700, 2, vp(pout), 500, None)),
            ("output at 2 mod 4", INV, lambda: L.melspec_resample_ragged_device(h, vp(pin), 1, po, pl, 2, vp(pout + 2), None, None)),
            ("misaligned before out_stride", INV, lambda: L.melspec_resample_uniform_device(h, vp(pin + 1), 1, 1400, 1400, 2, vp(pout), 3, None)),
            ("out_stride < out_len", INV, lambda: L.melspec_resample_uniform_device(h, vp(pin), 1, 1500, 1500, 2, vp(pout), 499, None)),
        ]
        for what, want, call in refused:
            assert call() == want, what
            assert _lib.last_error(), what
        assert L.melspec_resampler_synchronize(h, None) == _lib.OK
        assert np.all(d_out.download((1200,)) == SENTINEL), "a refused call wrote to its output"
        # the host call: capacity, NULL, alignment; nothing written
        out = np.full(1100, SENTINEL, np.float32)
        n = C.c_size_t(77)
        xp, op = x.ctypes.data_as(vp), out.ctypes.data_as(vp)
        assert L.melspec_resample_host(h, xp, 1, 3000, op, 999, C.byref(n)) == _lib.ERR_CAPACITY
        assert L.melspec_resample_host(h, xp, 3, 3000, op, 1000, C.byref(n)) == INV
        assert L.melspec_resample_host(h, None, 1, 3000, op, 1000, C.byref(n)) == INV
        assert L.melspec_resample_host(h, xp, 1, 3000, None, 1000, C.byref(n)) == INV
        assert L.melspec_resample_host(h, vp(x.ctypes.data + 1), 1, 2000, op, 1000, C.byref(n)) == INV
        assert n.value == 77 and np.all(out == SENTINEL)
        # what is fine: no clips, clips without a sample (no pointer is needed for them), a stride that is exactly out_len
        assert L.melspec_resample_uniform_device(h, None, 1, 0, 0, 0, None, 0, None) == _lib.OK
        assert L.melspec_resample_uniform_device(h, None, 0, 10, 0, 5, None, 0, None) == _lib.OK
        assert L.melspec_resample_ragged_device(h, None, 1, None, None, 0, None, None, None) == _lib.OK
        zero = np.zeros(2, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
        assert L.melspec_resample_ragged_device(h, vp(pin), 1, po, zero, 2, vp(pout), None, None) == _lib.OK
        assert L.melspec_resample_host(h, None, 1, 0, None, 0, C.byref(n)) == _lib.OK and n.value == 0
        assert L.melspec_resampler_synchronize(h, None) == _lib.OK
        assert np.all(d_out.download((1200,)) == SENTINEL)
        assert L.melspec_resample_uniform_device(h, vp(pin), 1, 1500, 1500, 2, vp(pout), 500, None) == _lib.OK
        assert L.melspec_resample_host(h, xp, 1, 3000, op, 1000, C.byref(n)) == _lib.OK and n.value == 1000
        rs.synchronize()
        got = d_out.download((1200,))
        assert np.all(got[1000:] == SENTINEL) and not np.any(got[:1000] == SENTINEL)
        same_bits(got[:500], rs.compute(x[:1500]), "uniform clip 0")
        same_bits(got[500:1000], rs.compute(x[1500:]), "uniform clip 1")
    finally:
        d.free()
        rs.close()
    # no usable device index
    bad = C.c_void_p()
    assert L.melspec_resampler_create(C.byref(bad), 10 ** 6, 48000, 16000) in (_lib.ERR_INVALID_ARG, _lib.ERR_UNAVAILABLE) and not bad.value
