"""NeMo / Parakeet frontend: the split output with 16-bit ends (melspec_blm_compute_{uniform,ragged}_device_split_io, _host_split_io,
melspec_blm_supports_split_io) -- int16 PCM in, f16 / bf16 rows out, f32 mean and 1 / std, no scratch rows and no second pass.

The yardstick is always an EXISTING call, never the new code: melspec_blm_compute_uniform_device_split on the batch converted by
`v as f32 / 32768.0` (tests/test_blm_split.py: run_split; tests/test_io_dtypes.py: to_f32).  The contract is the two existing contracts
joined:
  * rows: every element is the element the f32 split call writes, rounded to nearest even once (round_to); pad columns are +0;
  * mean / inv_std: THE BITS of the f32 split call -- the statistics of the f32 values, not of the rounded rows;
  * strides and offsets count elements; an int16 clip may start at an odd sample, 16-bit rows at an odd element;
  * the checks are those of the f32 split calls in their order, with the dtype codes in front and the alignment behind the NULL checks.
Every output sits between two guard bands of a sentinel no kernel computes (tests/test_io_dtypes.py: Fence).

Against the oracle (test 6) the bounds are derived, not tuned: the rows within 1e-4 (the f32 split call's own bound, tests/test_gpu_parity.py)
plus half an ulp of the row type at the element's magnitude (tests/test_blm_io_dtypes.py: half_ulp); the consumer's (rows - mean) * inv_std
within 1e-4 max(1, |z|) plus that half ulp times inv_std -- the rounding of a row carried through the consumer's multiply."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_blm_io_dtypes import half_ulp
from test_blm_split import TOL, VALID_FRAMES, f32, frontend, noise, run_split
from test_blm_split_ragged import assert_clip_bits, flatten, samples_for
from test_io_dtypes import (ERR_INVALID_ARG, ERR_UNSUPPORTED, NEW_COMBOS, OUT_BF16, OUT_F16, OUT_F32, OUT_NP, PCM_F32, PCM_S16, Fence, _upload, round_to, s16_noise,
                            s16_speech, s16_tone, to_f32, to_f64)

SYMBOLS = ["melspec_blm_supports_split_io", "melspec_blm_compute_uniform_device_split_io", "melspec_blm_compute_ragged_device_split_io",
           "melspec_blm_compute_host_split_io"]
U64P = C.POINTER(C.c_uint64)
NAME = {(PCM_S16, OUT_F32): "s16-f32", (PCM_F32, OUT_F16): "f32-f16", (PCM_F32, OUT_BF16): "f32-bf16", (PCM_S16, OUT_F16): "s16-f16", (PCM_S16, OUT_BF16): "s16-bf16"}


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(U64P)


def _vp(p):
    return None if p is None else C.c_void_p(p)


def s16_clips(jfk, n_clips, n, base=0):
    """int16 clips of three kinds, made on the host from seeds (tests/test_io_dtypes.py)"""
    make = (s16_noise, lambda c, m: s16_speech(jfk, c, m), s16_tone)
    return np.stack([make[(base + c) % 3](base + c, n) for c in range(n_clips)])


def as_pcm(s16, pcm):
    """the batch as the call's sample type: the int16 values, or their exact f32 conversion"""
    return s16 if pcm == PCM_S16 else to_f32(s16)


def call_uniform(gpu, fe, d_pcm, pcm, n, n_clips, d_rows, out, d_mean, d_inv_std, stream=None):
    return gpu._lib.lib().melspec_blm_compute_uniform_device_split_io(fe._h, _vp(d_pcm), pcm, n, n, n_clips, _vp(d_rows), out, _vp(d_mean), _vp(d_inv_std), stream)


def run_split_io(gpu, fe, clips, pcm, out):
    """clips [n_clips, n] of the sample type -> bits (rows [n_clips, n_mels, cols] of the row type, mean, inv_std [n_clips, n_mels]) of
    the three fenced outputs, every element written"""
    n_clips, n = clips.shape
    nm, cols = fe.config.n_mels, fe.padded_frames(n)
    d = _upload(gpu, clips)
    fr, fm, fs = Fence(gpu, n_clips * nm * cols, out), Fence(gpu, n_clips * nm, OUT_F32), Fence(gpu, n_clips * nm, OUT_F32)
    rc = call_uniform(gpu, fe, d.ptr, pcm, n, n_clips, fr.ptr, out, fm.ptr, fs.ptr)
    fe.synchronize()
    rows, mean, inv_std = fr.bits(), fm.bits(), fs.bits()          # (checks the guard bands)
    d.free()
    assert rc == 0, gpu._lib.lib().melspec_last_error()
    for name, b, f in (("mean", mean, fm), ("inv_std", inv_std, fs)):
        left = b == f.s
        assert not left.any(), f"{name}: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    left = rows == fr.s
    assert not left.any(), f"rows: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    return rows.reshape(n_clips, nm, cols), mean.reshape(n_clips, nm), inv_std.reshape(n_clips, nm)


def assert_rounded(got, want32, out, what):
    want = round_to(want32, out).reshape(got.shape)
    diff = got != want
    assert not diff.any(), f"{what}: {int(diff.sum())} row elements are not the f32 split call's, rounded once (first at {np.argwhere(diff)[0]})"


def assert_same(got, want, name, what):
    diff = got != want
    assert not diff.any(), f"{what}: {name} differs from the f32 split call's bits in {int(diff.sum())} elements (first at {np.argwhere(diff)[0]})"


# ---- Test 1: uniform bits --------------------------------------------------------------------------------------------------------------

_UNIFORM = {}


def uniform_yardstick(gpu, jfk, nm, mode, center, pad_to):
    """-> (int16 clips, the f32 split call's (rows, mean, inv_std) bits on their conversion): computed once per configuration, left unchanged"""
    key = (nm, mode, center, pad_to)
    if key not in _UNIFORM:
        s16 = s16_clips(jfk, 5, 16007)          # 101 / 97 valid frames: a block and a unit end inside the row
        fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
        _UNIFORM[key] = (s16, run_split(gpu, fe, to_f32(s16)))
        fe.close()
    return _UNIFORM[key]


@pytest.mark.gpu
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("pad_to", [0, 16])
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_uniform_rows_are_the_f32_split_rounded_once(gpu, jfk, nm, mode, pad_to, center):
    s16, (rows32, mean32, inv32) = uniform_yardstick(gpu, jfk, nm, mode, center, pad_to)
    fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
    valid = fe.num_frames(16007)
    for pcm, out in NEW_COMBOS:
        what = f"{nm} {mode} pad_to {pad_to} center {center} {NAME[pcm, out]}"
        assert gpu._lib.lib().melspec_blm_supports_split_io(fe._h, pcm, out) == 1
        rows, mean, inv_std = run_split_io(gpu, fe, as_pcm(s16, pcm), pcm, out)
        assert_rounded(rows, rows32, out, what)
        assert np.all(rows[:, :, valid:] == 0), f"{what}: pad columns are +0"
        assert_same(mean, mean32, "mean", what)
        assert_same(inv_std, inv32, "inv_std", what)
    # (F32, F32) through the new entry is the existing call
    rows, mean, inv_std = run_split_io(gpu, fe, to_f32(s16), PCM_F32, OUT_F32)
    fe.close()
    assert_same(rows, rows32, "rows", "f32-f32")
    assert_same(mean, mean32, "mean", "f32-f32")
    assert_same(inv_std, inv32, "inv_std", "f32-f32")


# ---- the ragged call --------------------------------------------------------------------------------------------------------------------

def flatten_as(clips, dtype):
    """test_blm_split_ragged's flatten -- one sample in front of each clip: odd and even offsets -- for clips of `dtype`"""
    if dtype == np.float32:
        return flatten(clips)
    lens = np.array([len(c) for c in clips], np.uint64)
    offs = (np.concatenate([[0], np.cumsum(lens + 1)[:-1]]) + 1).astype(np.uint64)
    flat = np.full(int(offs[-1] + lens[-1]) + 1, 8192, dtype)
    for o, c in zip(offs, clips):
        flat[int(o):int(o) + len(c)] = c
    return flat, offs, lens


def call_ragged(gpu, fe, d_pcm, pcm, offs, lens, n_clips, d_rows, out, rows_offs, d_mean, d_inv_std, stream=None):
    keep = [None if t is None else _u64(t) for t in (offs, lens, rows_offs)]
    tabs = [None if k is None else k[1] for k in keep]
    return gpu._lib.lib().melspec_blm_compute_ragged_device_split_io(fe._h, _vp(d_pcm), pcm, tabs[0], tabs[1], n_clips, _vp(d_rows), out, tabs[2], _vp(d_mean),
                                                                    _vp(d_inv_std), stream)


def run_ragged_split_io(gpu, fe, clips, pcm, out, rows_offs=None, span=None):
    """list of 1-D clips of the sample type -> ([rows bits [n_mels, cols_c] per clip], mean bits, inv_std bits [n_clips, n_mels], the f32
    sentinel): the three outputs fenced; every element of the rows' allocation that belongs to no clip must still be the sentinel, every
    element that does must have been written (tests/test_blm_split_ragged.py: run_ragged_split)"""
    nm, n = fe.config.n_mels, len(clips)
    cols = [fe.padded_frames(len(c)) for c in clips]
    sizes = [nm * c for c in cols]
    if rows_offs is None:
        at = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        span = int(sum(sizes))
    else:
        at = np.asarray(rows_offs, np.int64)
    flat, offs, lens = flatten_as(clips, np.int16 if pcm == PCM_S16 else np.float32)
    assert {int(o) & 1 for o, c in zip(offs, cols) if c} == {0, 1} or n < 3, "clips start at odd and at even samples"
    d = _upload(gpu, flat)
    fr, fm, fs = Fence(gpu, max(span, 1), out), Fence(gpu, n * nm, OUT_F32), Fence(gpu, n * nm, OUT_F32)
    rc = call_ragged(gpu, fe, d.ptr, pcm, offs, lens, n, fr.ptr, out, rows_offs, fm.ptr, fs.ptr)
    fe.synchronize()
    rows, mean, inv_std = fr.bits(), fm.bits(), fs.bits()          # (checks the guard bands)
    d.free()
    assert rc == 0, gpu._lib.lib().melspec_last_error()
    owned = np.zeros(max(span, 1), bool)
    res = []
    for a, size, c in zip(at, sizes, cols):
        assert not owned[a:a + size].any(), "the test's own offsets overlap"
        owned[a:a + size] = True
        res.append(rows[a:a + size].reshape(nm, c))
    left = (rows == fr.s) & owned
    assert not left.any(), f"rows: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    stray = (rows != fr.s) & ~owned
    assert not stray.any(), f"rows: {int(stray.sum())} elements between the clips' rows were written (first at {int(np.argmax(stray))})"
    return res, mean.reshape(n, nm), inv_std.reshape(n, nm), fm.s


# ---- Test 2: ragged bits at the edges --------------------------------------------------------------------------------------------------

_EDGE = {}


def edge_batch(gpu, jfk, nm, mode, center, pad_to):
    """test_blm_split_ragged's edge batch in int16 -> (clips, valid frames per clip, [(rows, mean, inv_std) bits of the uniform f32 split on
    the converted clip alone, or None for a frameless clip]); computed once per configuration, left unchanged"""
    key = (nm, mode, center, pad_to)
    if key not in _EDGE:
        order = np.random.default_rng(4).permutation(len(VALID_FRAMES))
        valid = [VALID_FRAMES[i] for i in order]
        clips = [s16_clips(jfk, 1, samples_for(v, center), base=300 + v)[0] for v in valid]
        valid.insert(6, 0)          # in the middle: a clip without a frame -- center = 0: 300 samples (fewer than n_fft); centred: no sample at all
        clips.insert(6, s16_noise(7, 0 if center else 300))
        fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
        want = []
        for v, x in zip(valid, clips):
            assert fe.num_frames(len(x)) == v
            if v == 0:
                want.append(None)
                continue
            rows, mean, inv_std = run_split(gpu, fe, to_f32(x)[None, :])
            want.append((rows[0].copy(), mean[0].copy(), inv_std[0].copy()))
        fe.close()
        _EDGE[key] = (clips, valid, want)
    return _EDGE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("pcm,out", [(PCM_S16, OUT_F16), (PCM_S16, OUT_BF16), (PCM_F32, OUT_F16), (PCM_S16, OUT_F32)], ids=lambda v: str(v))
@pytest.mark.parametrize("nm,mode,center,pad_to", [(nm, mode, center, pad_to) for nm in (80, 128) for mode in ("f64", "f32") for center, pad_to in ((True, 0), (False, 16))],
                         ids=lambda v: {True: "center", False: "nocenter"}.get(v, str(v)) if isinstance(v, bool) else str(v))
def test_ragged_clips_at_the_edges_with_caller_offsets(gpu, jfk, nm, mode, center, pad_to, pcm, out):
    """clips of VALID_FRAMES valid frames each, shuffled, a frameless clip in the middle; int16 clips at odd and even sample offsets; the
    rows in reverse clip order with gaps of 1, 3 and 64 elements in front of them, which puts 16-bit rows at odd elements.  Every clip is
    the uniform f32 split on the clip alone, rounded; gaps, fences and the frameless clip's statistics slots are untouched."""
    clips, valid, want = edge_batch(gpu, jfk, nm, mode, center, pad_to)
    fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
    offs, cur = [0] * len(clips), 0
    for k, c in enumerate(reversed(range(len(clips)))):
        cur += (1, 3, 64)[k % 3]
        offs[c] = cur
        cur += nm * fe.padded_frames(len(clips[c]))
    assert any(o & 1 for o in offs) and any(not o & 1 for o in offs)
    rows, mean, inv_std, sentinel = run_ragged_split_io(gpu, fe, [as_pcm(c, pcm) for c in clips], pcm, out, rows_offs=offs, span=cur + 3)
    fe.close()
    for c, (v, w) in enumerate(zip(valid, want)):
        what = f"{nm} {mode} pad_to {pad_to} center {center} {NAME[pcm, out]}, clip {c} ({v} valid frames)"
        if v == 0:
            assert rows[c].size == 0
            assert np.all(mean[c] == sentinel) and np.all(inv_std[c] == sentinel), f"{what}: the statistics slots of the frameless clip were written"
            continue
        assert_rounded(rows[c], w[0], out, what)
        assert np.all(rows[c][:, v:] == 0), f"{what}: pad columns are +0"
        assert_same(mean[c], w[1], "mean", what)
        assert_same(inv_std[c], w[2], "inv_std", what)


# ---- Test 3: past one trip of the grid --------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("pcm,out", [(PCM_S16, OUT_F16), (PCM_F32, OUT_BF16)], ids=["s16-f16", "f32-bf16"])
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_large_batch_past_one_trip_of_the_grid(gpu, nm, mode, pcm, out):
    """the 4099-clip batch of tests/test_blm_split_ragged.py (4096 clips of 12 lengths between 0.05 s and 0.6 s, three of 10 s) in int16,
    against one uniform f32 split call per distinct length; the same batch twice gives the same bits"""
    rng = np.random.default_rng(6)
    lengths = [800, 1600, 2400, 3200, 4000, 4799, 5600, 6400, 7200, 8000, 8800, 9600]
    lens = list(rng.choice(lengths, 4096))
    for at in (17, 2048, 4098):
        lens.insert(at, 160000)
    lens = np.array(lens)
    fe = frontend(gpu, nm, mode, pad_to=16 if nm == 80 else 0)
    clips = [None] * len(lens)
    want = [None] * len(lens)
    for n in sorted(set(lens.tolist())):
        idx = np.flatnonzero(lens == n)
        group = np.clip(np.rint(noise(n, (len(idx), n)) * 32768.0), -32768, 32767).astype(np.int16)
        rows, mean, inv_std = run_split(gpu, fe, to_f32(group))
        rows = round_to(rows, out).reshape(rows.shape)
        for k, c in enumerate(idx):
            clips[c] = as_pcm(group[k], pcm)
            want[c] = (rows[k], mean[k], inv_std[k])
    rows, mean, inv_std, _ = run_ragged_split_io(gpu, fe, clips, pcm, out)
    for c in range(len(lens)):
        assert_clip_bits((rows[c], mean[c], inv_std[c]), want[c], f"{nm} {mode} {NAME[pcm, out]}: clip {c} of {len(lens)} ({lens[c]} samples)")
    rows2, mean2, inv_std2, _ = run_ragged_split_io(gpu, fe, clips, pcm, out)
    fe.close()
    assert np.array_equal(mean, mean2) and np.array_equal(inv_std, inv_std2), "the same batch gave other statistics the second time"
    assert all(np.array_equal(a, b) for a, b in zip(rows, rows2)), "the same batch gave other rows the second time"


# ---- Test 4: digital silence -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_digital_silence(gpu, mode, out):
    """int16 zeros: inv_std is 1e5 exactly and the mean is the f32 call's mean -- the f32 value, not the rounded row"""
    fe = frontend(gpu, 128, mode)
    lens = (16000, 160, 4800, 7680, 33, 160000, 5120)
    clips = [np.zeros(n, np.int16) for n in lens]
    rows, mean, inv_std, _ = run_ragged_split_io(gpu, fe, clips, PCM_S16, out)
    rounds = 0
    for c, n in enumerate(lens):
        r32, m32, s32 = run_split(gpu, fe, np.zeros((1, n), np.float32))
        assert np.all(f32(inv_std[c]) == np.float32(1e5)), (c, f32(inv_std[c])[:4])
        assert_same(mean[c], m32[0], "mean", f"silence, clip {c}")
        assert_rounded(rows[c], r32[0], out, f"silence, clip {c}")
        rounds += int((to_f64(round_to(m32[0], out), out) != f32(m32[0]).astype(np.float64)).sum())
    fe.close()
    assert rounds > 0, "the silent rows' value is not representable in the row type: the mean is not the rounded row"


# ---- Test 5: non-finite input -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_a_nan_sample_stays_a_nan(gpu, mode, out):
    """one NaN f32 sample: the row elements of the frames it touches are NaN in the row type, everything else is the f32 call's rounding"""
    fe = frontend(gpu, 80, mode)
    clips = noise(11, (3, 16007))
    clips[1, 8000] = np.nan
    rows32, mean32, inv32 = run_split(gpu, fe, clips)
    rows, mean, inv_std = run_split_io(gpu, fe, clips, PCM_F32, out)
    fe.close()
    nan32 = np.isnan(f32(rows32))
    assert nan32[1].any() and not nan32[0].any() and not nan32[2].any()
    assert np.array_equal(np.isnan(to_f64(rows, out)), nan32), "a NaN of the f32 rows is a NaN of the 16-bit rows and nothing else is"
    want = round_to(rows32, out).reshape(rows.shape)
    assert np.array_equal(rows[~nan32], want[~nan32])
    for name, a, b in (("mean", mean, mean32), ("inv_std", inv_std, inv32)):
        nan = np.isnan(f32(b))
        assert np.array_equal(np.isnan(f32(a)), nan) and np.array_equal(a[~nan], b[~nan]), name


# ---- Test 6: the oracle, end to end -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("out,name", [(OUT_F16, "f16"), (OUT_BF16, "bf16")], ids=["f16", "bf16"])
@pytest.mark.parametrize("kw", [dict(), dict(n_mels=128, preemphasis=0.97)], ids=["80", "128-preemph"])
def test_python_entry_points_match_the_oracle(gpu, oracle, jfk, kw, out, name):
    """blm_compute_split_io and blm_compute_ragged_split_io on jfk and two synthetic clips, int16 in.  Rows: within 1e-4 + half an ulp of
    the row type at that magnitude of the oracle's raw rows on the converted samples.  On the rows whose f64 std is >= 0.5 the consumer's
    (rows - mean) * inv_std against the oracle's normalised rows: 1e-4 max(1, |z|) + half_ulp * inv_std -- the second term is the
    rounding of the rows carried through the consumer's multiply.  At least one gated row per clip."""
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    cfg_raw = oracle.blm_default_config(**kw)
    cfg_norm = oracle.blm_default_config(normalize_per_feature=1, **kw)
    q = lambda x: np.clip(np.rint(x.astype(np.float64) * (0.9 / np.abs(x).max()) * 32768.0), -32768, 32767).astype(np.int16)
    clips = [q(jfk), q(oracle.synth_pcm(2, 16007)), q(oracle.synth_pcm(5, 48000))]
    ragged = gpu.blm_compute_ragged_split_io(fe, clips, name)
    assert len(ragged) == len(clips)
    for x, from_batch in zip(clips, ragged):
        x32 = to_f32(x)
        raw_want, valid = oracle.blm_compute(x32, cfg_raw, True)
        want, _ = oracle.blm_compute(x32, cfg_norm, True)
        single = gpu.blm_compute_split_io(fe, x, name)
        for what, (rows, mean, inv_std) in (("host", single), ("ragged", from_batch)):
            assert rows.shape == want.shape and fe.num_frames(len(x)) == valid and mean.dtype == np.float32 and inv_std.dtype == np.float32
            r = to_f64(rows.view(OUT_NP[out]), out)
            hu = half_ulp(raw_want, out)
            over = np.abs(r - raw_want) - (TOL + hu)
            got = np.zeros_like(r)
            got[:, :valid] = (r[:, :valid] - mean[:, None].astype(np.float64)) * inv_std[:, None].astype(np.float64)
            std = raw_want[:, :valid].astype(np.float64).std(axis=1, ddof=1)
            good = std >= 0.5
            gated = int(good.sum())
            bound = TOL * np.maximum(1.0, np.abs(want[good])) + hu[good] * inv_std[good, None].astype(np.float64)
            bound[:, valid:] = 0.0
            d = np.abs(got[good] - want[good]) - bound
            print(f"{kw} {name} {what} {len(x)} samples: rows worst over the bound {float(over.max()):.3e}; {gated} rows gated, worst over the bound "
                  f"{float(d.max()) if gated else float('nan'):.3e}")
            assert over.max() <= 0, float(over.max())
            assert gated > 0
            assert d.max() <= 0, float(d.max())
        for a, b in zip(single, from_batch):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "the host call and the ragged call disagree on a clip"
    empty = gpu.blm_compute_ragged_split_io(fe, [clips[1], np.zeros(0, np.int16)], name)
    assert empty[1][0].shape == (fe.config.n_mels, 0) and empty[1][1] is None and empty[1][2] is None
    fe.close()


# ---- Test 7: refusals write nothing -----------------------------------------------------------------------------------------------------

def _refused(gpu, fe, clips, pcm=PCM_S16, out=OUT_F16, null=(), n_clips=None, ragged=True, odd=()):
    """the call with the arguments named in `null` passed as NULL and those in `odd` one byte off -> its status; none of the three fenced
    outputs may have been written.  clips: int16, equal lengths for the uniform call"""
    nm, n = fe.config.n_mels, len(clips)
    ok_out = out if out in OUT_NP else OUT_F16
    flat, offs, lens = flatten_as([as_pcm(c, pcm if pcm in (PCM_F32, PCM_S16) else PCM_S16) for c in clips], np.float32 if pcm == PCM_F32 else np.int16)
    d = _upload(gpu, flat if ragged else np.stack(clips))
    fr = Fence(gpu, max(sum(nm * fe.padded_frames(len(c)) for c in clips), 1), ok_out)
    fm, fs = Fence(gpu, n * nm, OUT_F32), Fence(gpu, n * nm, OUT_F32)
    arg = dict(pcm=d.ptr, offs=offs, lens=lens, rows=fr.ptr, mean=fm.ptr, inv_std=fs.ptr)
    for k in null:
        arg[k] = None
    for k in odd:
        arg[k] += 1
    cnt = n if n_clips is None else n_clips
    if ragged:
        rc = call_ragged(gpu, fe, arg["pcm"], pcm, arg["offs"], arg["lens"], cnt, arg["rows"], out, None, arg["mean"], arg["inv_std"])
    else:
        rc = call_uniform(gpu, fe, arg["pcm"], pcm, len(clips[0]), cnt, arg["rows"], out, arg["mean"], arg["inv_std"])
    fe.synchronize()
    for name, f in (("rows", fr), ("mean", fm), ("inv_std", fs)):
        b = f.bits()
        assert np.all(b == f.s), f"{name}: a call that computes nothing wrote {int((b != f.s).sum())} elements"
    d.free()
    return rc


@pytest.mark.gpu
def test_refusals_write_nothing(gpu):
    last = lambda: gpu._lib.lib().melspec_last_error().decode()
    lib = gpu._lib.lib()
    clips = [s16_noise(c, 4000) for c in range(2)]
    for kw in (dict(n_mels=40), dict(n_mels=80, n_fft=1024, win_length=800, hop_length=256), dict(n_mels=80, n_fft=512, win_length=320)):
        fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
        assert not gpu.blm_supports_split_io(fe, PCM_S16, OUT_F16) and not gpu.blm_supports_split_io(fe, PCM_F32, OUT_F32), kw
        for ragged in (True, False):
            assert _refused(gpu, fe, clips, ragged=ragged) == ERR_UNSUPPORTED
            msg = last()
            assert "split output" in msg and f"n_mels = {kw['n_mels']}" in msg and f"n_fft = {kw.get('n_fft', 512)}" in msg, msg
            # unsupported comes before everything but the NULL context and the dtype codes: also without clips, tables or pointers
            assert _refused(gpu, fe, clips, null=("offs", "lens", "pcm", "rows", "mean", "inv_std"), n_clips=0, ragged=ragged) == ERR_UNSUPPORTED
        with pytest.raises(Exception):
            gpu.blm_compute_ragged_split_io(fe, clips, "f16")
        with pytest.raises(Exception):
            gpu.blm_compute_split_io(fe, clips[0], "bf16")
        fe.close()
    for nm, mode in ((80, "f64"), (128, "f32")):
        fe = frontend(gpu, nm, mode, center=False)
        for pcm, out in NEW_COMBOS + [(PCM_F32, OUT_F32)]:
            assert lib.melspec_blm_supports_split_io(fe._h, pcm, out) == 1
        for pcm, out in ((2, OUT_F16), (-1, OUT_F16), (PCM_S16, 3), (PCM_S16, -1)):
            assert lib.melspec_blm_supports_split_io(fe._h, pcm, out) == 0
            for ragged in (True, False):
                assert _refused(gpu, fe, clips, pcm=pcm, out=out, ragged=ragged) == ERR_INVALID_ARG, (pcm, out)
                assert "dtype must be" in last()
        for ragged in (True, False):
            assert _refused(gpu, fe, clips, null=("offs", "lens", "pcm", "rows", "mean", "inv_std"), n_clips=0, ragged=ragged) == 0          # no clips: OK
            for ptr in ("pcm", "rows", "mean", "inv_std"):
                assert _refused(gpu, fe, clips, null=(ptr,), ragged=ragged) == ERR_INVALID_ARG, ptr
                assert "NULL" in last()
            # 16-bit types at odd addresses
            for ptr in ("pcm", "rows"):
                assert _refused(gpu, fe, clips, odd=(ptr,), ragged=ragged) == ERR_INVALID_ARG, ptr
                assert "aligned" in last()
            assert _refused(gpu, fe, clips, pcm=PCM_F32, out=OUT_BF16, odd=("rows",), ragged=ragged) == ERR_INVALID_ARG
            # no valid frame in the whole batch (center = 0, fewer than n_fft samples): OK, nothing written, the pointers are not looked at
            short = [s16_noise(c, 300) for c in range(3)]
            assert _refused(gpu, fe, short, ragged=ragged) == 0
            assert _refused(gpu, fe, short, null=("pcm", "rows", "mean", "inv_std"), ragged=ragged) == 0
        for tab in ("offs", "lens"):
            assert _refused(gpu, fe, clips, null=(tab,)) == ERR_INVALID_ARG
            assert "offset/length" in last()
        assert _refused(gpu, fe, [s16_noise(c, 300) for c in range(3)], null=("offs",)) == ERR_INVALID_ARG              # the tables are looked at
        fe.close()


# ---- Test 8: ordering ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_two_calls_back_to_back_on_one_stream(gpu, jfk, nm, mode):
    """two calls of different row types on one stream with no synchronise between them: both give the bits of test 1 -- the partials
    scratch is reused in stream order"""
    s16, (rows32, mean32, inv32) = uniform_yardstick(gpu, jfk, nm, mode, True, 0)
    fe = frontend(gpu, nm, mode, pad_to=0, center=True, preemphasis=0.97)
    n_clips, n = s16.shape
    cols = fe.padded_frames(n)
    d = _upload(gpu, s16)
    outs = []
    for out in (OUT_F16, OUT_BF16):
        fr, fm, fs = Fence(gpu, n_clips * nm * cols, out), Fence(gpu, n_clips * nm, OUT_F32), Fence(gpu, n_clips * nm, OUT_F32)
        assert call_uniform(gpu, fe, d.ptr, PCM_S16, n, n_clips, fr.ptr, out, fm.ptr, fs.ptr) == 0
        outs.append((out, fr, fm, fs))
    fe.synchronize()
    for out, fr, fm, fs in outs:
        assert_rounded(fr.bits().reshape(rows32.shape), rows32, out, f"back to back, out {out}")
        assert_same(fm.bits().reshape(mean32.shape), mean32, "mean", f"back to back, out {out}")
        assert_same(fs.bits().reshape(inv32.shape), inv32, "inv_std", f"back to back, out {out}")
    d.free()
    fe.close()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------------

def test_split_io_symbols_everywhere():
    """the four entry points resolve in the built library and are declared in the header, the ctypes table, the C++ wrapper and the Rust
    shim; the Python functions are exported; the ABI version is still 1 and the header is still C99"""
    from mel_spec_amd import _lib
    import mel_spec_amd
    lib = _lib.lib()
    header_path = os.path.join(ROOT, "include", "melspec_hip.h")
    header = open(header_path).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    wrapper = open(os.path.join(ROOT, "include", "melspec_hip.hpp")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    for sym in SYMBOLS:
        assert getattr(lib, sym) is not None
        assert sym in _lib.SIGNATURES
        assert re.search(rf"\b{sym}\s*\(", header), sym
        assert f'"{sym}"' in table, sym
        assert re.search(rf"\b{sym}\s*\(", wrapper), sym
        assert re.search(rf"\bfn {sym}\s*\(", shim), sym
    assert "int16 PCM in or 16-bit rows out for the split" not in header and "no 16-bit ends" not in header
    for name in ("blm_supports_split_io", "blm_compute_uniform_device_split_io", "blm_compute_split_io", "blm_compute_ragged_device_split_io",
                 "blm_compute_ragged_split_io"):
        assert callable(getattr(mel_spec_amd, name)) and name in mel_spec_amd.__all__, name
    assert lib.melspec_abi_version() == 1
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-x", "c", header_path])


def test_split_io_null_context_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    tab, tp = _u64([0])
    ln, lp = _u64([1024])
    n = C.c_size_t(0)
    assert lib.melspec_blm_supports_split_io(None, PCM_S16, OUT_F16) == 0
    assert lib.melspec_blm_compute_uniform_device_split_io(None, p, PCM_S16, 1024, 1024, 1, p, OUT_F16, p, p, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_compute_ragged_device_split_io(None, p, PCM_S16, tp, lp, 1, p, OUT_F16, None, p, p, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_compute_ragged_device_split_io(None, None, 7, None, None, 0, None, 7, None, None, None, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_compute_host_split_io(None, p, PCM_S16, 1024, p, OUT_F16, 1024, buf.ctypes.data_as(C.POINTER(C.c_float)),
                                                 buf.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n), C.byref(n)) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert np.all(buf == 0)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_split_io_arguments_and_side_table_on_the_host(tmp_path, sanitize):
    """the arithmetic half of the host side (mel_spec_amd/csrc/blm_split_io_plan.hpp: the dtype codes, the argument verdicts in their
    order, the side table's index) as a stand-alone program, plain and with -fsanitize=address,undefined: tests/cpp/blm_split_io_host.cpp"""
    exe = tmp_path / "blm_split_io_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blm_split_io_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("blm_split_io_host: ok"), p.stdout + p.stderr
