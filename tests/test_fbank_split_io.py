"""Kaldi fbank, the split output for ragged batches and with 16-bit ends: melspec_fbank_compute_ragged_device_split (f32) and
melspec_fbank_compute_uniform_device_split_io / _ragged_device_split_io / _host_split_io (int16 PCM in, f16 / bf16 rows out, f32 means).

The yardsticks are existing calls or the oracle, never the new code, and exact, so nothing here is tuned:
  * rows: the f32 elements an object with the same config and apply_cmn = 0 writes through melspec_fbank_compute_uniform_device /
    _ragged_device on the batch converted by `v as f32 / 32768.0`, each rounded to nearest even once (tests/test_io_dtypes.py: round_to);
  * means: THE BITS melspec_fbank_compute_uniform_device_split gives for that clip -- alone (n_clips = 1), or in launches of 40 clips
    (wave kernel + cmn_kernel, never fbank512_clip_kernel) --, +0.0 for a clip without a frame;
  * the f32 ragged split: rows - means in f32 = the bits of melspec_fbank_compute_ragged_device;
  * against the oracle: the fused fbank gate (TOL = 1e-4) + half a unit in the last place of the row type for the rows, and for the means
    the derived bound of tests/test_fbank_tiny_clips.py::test_tiny_uniform_split, 1e-4 + F x 2^-24 x max|row|.
Every output sits between two guard bands of a sentinel no kernel computes (tests/test_io_dtypes.py: Fence): every element is written,
gaps and bands are untouched.  Frames = (n - 400) / 160 + 1."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_io_dtypes import (ERR_CAPACITY, ERR_INVALID_ARG, ERR_UNSUPPORTED, NEW_COMBOS, OUT_BF16, OUT_F16, OUT_F32, PCM_F32, PCM_S16, SENTINEL, Fence,
                            _upload, round_to, s16_noise, s16_speech, to_f32, to_f64)
from test_blm_io_dtypes import half_ulp, same
from test_fbank_io_dtypes import EDGE_LENS, NM, RAGGED_LENS, TOL, _mixed, ragged_flat, ragged_tables
from test_fbank_tiny_clips import FL, FS, SMALL, ragged_tiny_batch, shares, takes_clip_kernel_ragged, takes_clip_kernel_uniform
from test_whole_batch import THREADS, _cus

SPLIT_SYMBOLS = ["melspec_fbank_supports_split_io", "melspec_fbank_compute_ragged_device_split", "melspec_fbank_compute_uniform_device_split_io",
                 "melspec_fbank_compute_ragged_device_split_io", "melspec_fbank_compute_host_split_io"]
SPLIT_FUNCTIONS = ["fbank_supports_split_io", "fbank_compute_ragged_device_split", "fbank_compute_uniform_device_split_io",
                   "fbank_compute_ragged_device_split_io", "fbank_compute_split_io", "fbank_compute_ragged_split_io"]
ALL_COMBOS = [(PCM_F32, OUT_F32)] + NEW_COMBOS
IN_BYTES = {PCM_F32: 4, PCM_S16: 2}
S_MEANS = np.uint32(SENTINEL[OUT_F32])


# ---- runners: everything fenced, bits out ------------------------------------------------------------------------------------------

def pair(gpu, **kw):
    """(the object under test, its apply_cmn = 0 twin: the yardstick of the rows)"""
    return gpu.Fbank(gpu.FbankConfig(**kw)), gpu.Fbank(gpu.FbankConfig(apply_cmn=False, **kw))


def written(f, what):
    bits = f.bits()
    left = bits == f.s
    assert not left.any(), f"{what}: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    return bits


def plain_uniform(gpu, raw, f32):
    """the f32 call of the apply_cmn = 0 object -> bits [n_clips, frames, 80]"""
    n_clips, n = f32.shape
    nf = raw.num_frames(n)
    d, f = _upload(gpu, f32), Fence(gpu, n_clips * nf * NM, OUT_F32)
    raw.compute_uniform_device(d.ptr, n, n, n_clips, f.ptr)
    raw.synchronize()
    d.free()
    return written(f, "plain rows").reshape(n_clips, nf, NM)


def f32_split_uniform(gpu, fb, f32, per_launch=None):
    """melspec_fbank_compute_uniform_device_split (existing), in launches of per_launch clips -> the means' bits [n_clips, 80]"""
    n_clips, n = f32.shape
    nf = fb.num_frames(n)
    per = per_launch or n_clips
    d, rows, means = _upload(gpu, f32), Fence(gpu, n_clips * nf * NM, OUT_F32), Fence(gpu, n_clips * NM, OUT_F32)
    for c0 in range(0, n_clips, per):
        k = min(per, n_clips - c0)
        fb.compute_uniform_device_split(d.ptr + c0 * n * 4, n, n, k, rows.ptr + c0 * nf * NM * 4, means.ptr + c0 * NM * 4)
    fb.synchronize()
    d.free()
    rows.bits()
    return written(means, "f32 split means").reshape(n_clips, NM)


def split_uniform(gpu, fb, clips, pcm, out):
    """the new uniform call -> (rows' bits [n_clips, frames, 80], means' bits [n_clips, 80])"""
    n_clips, n = clips.shape
    nf = fb.num_frames(n)
    d, rows, means = _upload(gpu, clips), Fence(gpu, n_clips * nf * NM, out), Fence(gpu, n_clips * NM, OUT_F32)
    gpu.fbank_compute_uniform_device_split_io(fb, d.ptr, pcm, n, n, n_clips, rows.ptr, out, means.ptr)
    fb.synchronize()
    d.free()
    return written(rows, f"split rows ({pcm}, {out})").reshape(n_clips, nf, NM), written(means, f"split means ({pcm}, {out})").reshape(n_clips, NM)


def alone_means(gpu, fb, flat32, offs, lens):
    """every clip through the existing uniform f32 split ALONE (n_clips = 1) -> the means' bits [n_clips, 80]; +0.0 without a frame"""
    frames = [fb.num_frames(int(n)) for n in lens]
    d, rows, means = _upload(gpu, flat32), Fence(gpu, max(sum(frames), 1) * NM, OUT_F32), Fence(gpu, len(lens) * NM, OUT_F32)
    cur = 0
    for c, (o, n) in enumerate(zip(offs, lens)):
        fb.compute_uniform_device_split(d.ptr + int(o) * 4, int(n), int(n), 1, rows.ptr + cur * NM * 4, means.ptr + c * NM * 4)
        cur += frames[c]
    fb.synchronize()
    d.free()
    rows.bits()
    return written(means, "alone means").reshape(len(lens), NM)


def ragged_call(gpu, fb, flat, offs, lens, frames, oo, total, gaps, pcm, out, how, packed=False):
    """how: "plain" = melspec_fbank_compute_ragged_device (f32), "split" = the new f32 ragged split, "io" = the new _split_io call
    -> (the clips' rows' bits, concatenated; the means' bits [n_clips, 80] or None); gaps and guard bands checked"""
    if packed:
        oo = np.concatenate([[0], np.cumsum([k * NM for k in frames])[:-1]]).astype(np.uint64)
        total, gaps = int(sum(frames)) * NM, []
    ln = np.array(lens, np.uint64)
    d, f, m = _upload(gpu, flat), Fence(gpu, total, out), Fence(gpu, len(lens) * NM, OUT_F32)
    if how == "plain":
        fb.compute_ragged_device(d.ptr, offs, ln, f.ptr, None if packed else oo)
    elif how == "split":
        gpu.fbank_compute_ragged_device_split(fb, d.ptr, offs, ln, f.ptr, m.ptr, None if packed else oo)
    else:
        gpu.fbank_compute_ragged_device_split_io(fb, d.ptr, pcm, offs, ln, f.ptr, out, m.ptr, None if packed else oo)
    fb.synchronize()
    d.free()
    bits = f.bits()
    for a, b in gaps:
        assert np.all(bits[a:b] == f.s), f"ragged {how} ({pcm}, {out}): the gap [{a}, {b}) between two outputs was written"
    res = []
    for c, k in enumerate(frames):
        piece = bits[int(oo[c]):int(oo[c]) + k * NM]
        assert not (piece == f.s).any(), f"ragged {how} ({pcm}, {out}): clip {c}: {int((piece == f.s).sum())} elements never written"
        res.append(piece)
    assert int((bits != f.s).sum()) == int(sum(frames)) * NM, f"ragged {how} ({pcm}, {out}): elements outside the clips' rows were written"
    rows = np.concatenate(res) if res else np.zeros(0, f.dt)
    if how == "plain":
        m.buf.free()
        return rows, None
    return rows, written(m, f"ragged {how} means ({pcm}, {out})").reshape(len(lens), NM)


def check_means(got, want, what):
    diff = np.flatnonzero(np.any(got != want, axis=1))
    assert diff.size == 0, f"{what}: the means of {diff.size} of {got.shape[0]} clips differ from the f32 split's bits, first clip {int(diff[0])}: " \
                           f"{got[diff[0]][:4]} != {want[diff[0]][:4]}"


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_split_symbols_everywhere():
    """the five entry points resolve in the built library and are declared in the header, the ctypes table and the Rust shim; the ABI
    version stays 1; the module-level functions are exported"""
    import mel_spec_amd as M
    from mel_spec_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "melspec_hip.h")).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    for name in SPLIT_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f'"{name}"' in table, name
        assert re.search(rf"\bfn {name}\s*\(", shim), name
    assert lib.melspec_abi_version() == 1
    for name in SPLIT_FUNCTIONS:
        assert callable(getattr(M, name)) and name in M.__all__, name
    assert "ragged Kaldi split" not in header and "ragged form of the Kaldi split" not in header


def test_split_null_object_and_bad_codes_need_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.int16)
    p = buf.ctypes.data_as(C.c_void_p)
    for pcm, out in ALL_COMBOS:
        assert lib.melspec_fbank_supports_split_io(None, pcm, out) == 0
    assert lib.melspec_fbank_compute_ragged_device_split(None, p, None, None, 1, p, None, p, None) == ERR_INVALID_ARG
    assert b"fbank is NULL" in lib.melspec_last_error()
    assert lib.melspec_fbank_compute_uniform_device_split_io(None, p, PCM_S16, 1024, 1024, 1, p, OUT_F16, p, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_ragged_device_split_io(None, p, PCM_S16, None, None, 1, p, OUT_F16, None, p, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_host_split_io(None, p, PCM_S16, 1024, p, OUT_F16, 1024, None, None) == ERR_INVALID_ARG
    assert b"fbank is NULL" in lib.melspec_last_error()
    # the NULL object is reported in front of a bad dtype code
    assert lib.melspec_fbank_compute_uniform_device_split_io(None, p, 7, 1024, 1024, 1, p, 9, p, None) == ERR_INVALID_ARG
    assert b"fbank is NULL" in lib.melspec_last_error()


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

CONFIGS = {"default": {}, "no-preemphasis": dict(preemphasis=0.0), "linear": dict(use_log_fbank=False), "shift-12.5ms": dict(frame_shift_ms=12.5)}


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", list(CONFIGS), ids=list(CONFIGS))
def test_uniform_bits(gpu, cfg):
    """1. three clips of every edge length (0, 1, 2, 4, 5, 32, 33 and 98 frames at the default shift), the five combinations: the rows are
    the rounded rows of the apply_cmn = 0 f32 call on the converted batch, the means the bits of the f32 split call; without a frame no
    row is written and the means are +0.0"""
    fb, raw = pair(gpu, **CONFIGS[cfg])
    for pcm, out in ALL_COMBOS:
        assert gpu.fbank_supports_split_io(fb, pcm, out)
    seen = set()
    for n in EDGE_LENS:
        s16 = _mixed(3, n, base=n % 7)
        f32 = to_f32(s16)
        nf = fb.num_frames(n)
        seen.add(nf)
        if nf == 0:
            for pcm, out in NEW_COMBOS:
                d, rows, means = _upload(gpu, s16 if pcm == PCM_S16 else f32), Fence(gpu, 4096, out), Fence(gpu, 3 * NM, OUT_F32)
                gpu.fbank_compute_uniform_device_split_io(fb, d.ptr, pcm, n, n, 3, rows.ptr, out, means.ptr)
                fb.synchronize()
                d.free()
                assert np.all(rows.bits() == rows.s), f"n={n} ({pcm}, {out}): rows were written for clips without a frame"
                assert not means.bits().any(), f"n={n} ({pcm}, {out}): the means of clips without a frame are not +0.0"
            continue
        want_rows = plain_uniform(gpu, raw, f32)
        want_means = f32_split_uniform(gpu, fb, f32)
        for pcm, out in NEW_COMBOS:
            rows, means = split_uniform(gpu, fb, s16 if pcm == PCM_S16 else f32, pcm, out)
            same(rows, want_rows, out, f"{cfg} n={n} ({pcm}, {out}) rows")
            check_means(means, want_means, f"{cfg} n={n} ({pcm}, {out})")
    if cfg != "shift-12.5ms":
        assert seen == {0, 1, 2, 4, 5, 32, 33, 98}
    fb.close(); raw.close()


TINY_F = (1, 5, 13, 29, 33, 36)


@pytest.mark.gpu
@pytest.mark.parametrize("F", TINY_F)
def test_many_tiny_clips_per_workgroup(gpu, F):
    """2. the parity-slot hazard: 5 cus - cus / 8 clips of F frames -- every workgroup takes at least three, so a parity slot of the
    kernel's LDS block is reused, and below eight units some waves have an empty share and run ahead -- (S16, F16) and (F32, BF16).
    Means: the bits of the f32 uniform split in launches of 40 clips (wave kernel + cmn_kernel); rows: the rounded apply_cmn = 0 rows."""
    assert [sum(1 for s in shares(f) if s == 0) for f in TINY_F] == [7, 6, 4, 0, 0, 0]
    cus = _cus()
    n_clips = 5 * cus - cus // 8
    assert n_clips // cus >= 3 and takes_clip_kernel_uniform(n_clips, cus, NM) and not takes_clip_kernel_uniform(SMALL, cus, NM)
    n = FL + (F - 1) * FS
    fb, raw = pair(gpu)
    assert fb.num_frames(n) == F
    s16 = np.stack([s16_noise(7000 + 37 * F + c, n) for c in range(n_clips)])
    f32 = to_f32(s16)
    want_rows = plain_uniform(gpu, raw, f32)
    want_means = f32_split_uniform(gpu, fb, f32, SMALL)
    for src, pcm, out in ((s16, PCM_S16, OUT_F16), (f32, PCM_F32, OUT_BF16)):
        rows, means = split_uniform(gpu, fb, src, pcm, out)
        bad = np.flatnonzero(np.any(means != want_means, axis=1))
        assert bad.size == 0, f"F={F} ({pcm}, {out}): the means of {bad.size} of {n_clips} clips differ from the two-kernel path's bits: first clip " \
                              f"{int(bad[0])} (workgroup {int(bad[0]) % cus}, its clip no. {int(bad[0]) // cus}), shares {shares(F)}"
        same(rows, want_rows, out, f"F={F} ({pcm}, {out}) rows")
    fb.close(); raw.close()


@pytest.mark.gpu
@pytest.mark.parametrize("packed", [False, True], ids=["gapped", "packed"])
def test_ragged_edge_lengths(gpu, packed):
    """3a. RAGGED_LENS -- odd and even sample starts, foreign samples between the clips, odd element offsets and gaps (or packed) --, the
    f32 ragged split and the five combinations.  Per clip: the means are the uniform f32 split's bits of that clip ALONE, the rows the
    rounded rows of melspec_fbank_compute_ragged_device on the apply_cmn = 0 object; clips without a frame get +0.0 means and no rows"""
    fb, raw = pair(gpu)
    lens = RAGGED_LENS
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    flat16 = ragged_flat(lens, offs, n_samples)
    flat32 = to_f32(flat16)
    tabs = (offs, lens, frames, oo, total, gaps)
    want_rows, _ = ragged_call(gpu, raw, flat32, *tabs, PCM_F32, OUT_F32, "plain", packed)
    want_means = alone_means(gpu, fb, flat32, offs, lens)
    assert frames.count(0) >= 4 and not want_means[[c for c, k in enumerate(frames) if k == 0]].any()
    rows, means = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "split", packed)
    assert np.array_equal(rows, want_rows), "f32 ragged split: the rows are not the apply_cmn = 0 rows"
    check_means(means, want_means, "f32 ragged split")
    for pcm, out in ALL_COMBOS:
        rows, means = ragged_call(gpu, fb, flat16 if pcm == PCM_S16 else flat32, *tabs, pcm, out, "io", packed)
        same(rows, want_rows, out, f"ragged ({pcm}, {out}) rows")
        check_means(means, want_means, f"ragged ({pcm}, {out})")
    fb.close(); raw.close()


def _tiny(gpu, fb, K):
    """ragged_tiny_batch(cus, K) as int16 noise, packed back to back -> (flat16, tables)"""
    cus = _cus()
    lens = ragged_tiny_batch(cus, K)
    frames = [fb.num_frames(n) for n in lens]
    assert frames.count(0) == K and len(lens) == 5 * cus + K and takes_clip_kernel_ragged(frames, cus, NM)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    rng = np.random.default_rng(900 + K)
    flat16 = (rng.integers(-32768, 32768, int(sum(lens)) + 8, dtype=np.int32) >> 2).astype(np.int16)
    return flat16, (offs, lens, frames, None, 0, [])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 64])
def test_ragged_ticket_ring_16bit(gpu, K):
    """3b. 5 x cus tiny clips and K clips without a frame scattered through them, (S16, F16): the ticket ring.  Per clip the means of the
    uniform f32 split of that clip alone, the rounded apply_cmn = 0 rows, +0.0 means without a frame; a second run gives the same bits"""
    fb, raw = pair(gpu)
    flat16, tabs = _tiny(gpu, fb, K)
    flat32 = to_f32(flat16)
    want_rows, _ = ragged_call(gpu, raw, flat32, *tabs, PCM_F32, OUT_F32, "plain", True)
    want_means = alone_means(gpu, fb, flat32, tabs[0], tabs[1])
    rows, means = ragged_call(gpu, fb, flat16, *tabs, PCM_S16, OUT_F16, "io", True)
    same(rows, want_rows, OUT_F16, f"tiny ragged K={K} rows")
    check_means(means, want_means, f"tiny ragged K={K}")
    rows2, means2 = ragged_call(gpu, fb, flat16, *tabs, PCM_S16, OUT_F16, "io", True)
    assert np.array_equal(rows, rows2) and np.array_equal(means, means2), "a second run gives other bits"
    fb.close(); raw.close()


@pytest.mark.gpu
def test_ragged_f32_split_either_side_of_the_clip_route(gpu):
    """3c + 4. the f32 ragged split on ragged_tiny_batch(cus, 9): once whole (by clip: fbank512_clip_kernel publishes the means) and once in
    slices below clip_ragged_ok (wave kernel + cmn_kernel): the same bits, the means of every clip alone.  And the consumer identity on
    both routes: rows - means in f32 = the bits melspec_fbank_compute_ragged_device stores."""
    cus = _cus()
    fb, raw = pair(gpu)
    flat16, tabs = _tiny(gpu, fb, 9)
    flat32 = to_f32(flat16)
    offs, lens, frames = tabs[0], tabs[1], tabs[2]
    want_rows, _ = ragged_call(gpu, raw, flat32, *tabs, PCM_F32, OUT_F32, "plain", True)
    fused, _ = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "plain", True)
    want_means = alone_means(gpu, fb, flat32, offs, lens)
    rows, means = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "split", True)
    assert np.array_equal(rows, want_rows), "by clip: the rows are not the apply_cmn = 0 rows"
    check_means(means, want_means, "f32 ragged split by clip")
    sub = (rows.view(np.float32).reshape(-1, NM) - np.repeat(means.view(np.float32), frames, axis=0)).astype(np.float32).view(np.uint32).reshape(-1)
    assert np.array_equal(sub, fused), "by clip: rows - means is not what melspec_fbank_compute_ragged_device stores"
    step = cus + cus // 2
    starts = np.concatenate([[0], np.cumsum(frames)]) * NM
    for c0 in range(0, len(lens), step):
        sl = slice(c0, c0 + step)
        assert not takes_clip_kernel_ragged(frames[sl], cus, NM)
        r, m = ragged_call(gpu, fb, flat32, offs[sl], lens[sl], frames[sl], None, 0, [], PCM_F32, OUT_F32, "split", True)
        assert np.array_equal(r, rows[starts[c0]:starts[min(c0 + step, len(lens))]]), f"clips {c0}..: the rows depend on the route"
        check_means(m, means[sl], f"clips {c0}.. below clip_ragged_ok")
    fb.close(); raw.close()


@pytest.mark.gpu
def test_consumer_identity_on_edge_lengths(gpu):
    """4. the f32 ragged split on RAGGED_LENS (gapped, odd offsets: the wave kernel + cmn_kernel): (rows - means).astype(f32) has the bits of
    melspec_fbank_compute_ragged_device"""
    fb = gpu.Fbank()
    lens = RAGGED_LENS
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    flat32 = to_f32(ragged_flat(lens, offs, n_samples))
    tabs = (offs, lens, frames, oo, total, gaps)
    fused, _ = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "plain")
    rows, means = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "split")
    sub = (rows.view(np.float32).reshape(-1, NM) - np.repeat(means.view(np.float32), frames, axis=0)).astype(np.float32).view(np.uint32).reshape(-1)
    assert np.array_equal(sub, fused)
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
def test_against_the_oracle(gpu, oracle, jfk, out):
    """5. the JFK clip whole (1098 frames) and eight noise clips of 1 s in one ragged batch, (S16, 16-bit), against the oracle with
    apply_cmn = 0 on the exactly converted samples.  Rows: TOL = 1e-4 (the fused fbank gate) + half a unit in the last place of the row
    type.  Means: 1e-4 + F x 2^-24 x max|row| around the f64 column mean of the oracle's rows -- the rows' exact mean is within 1e-4 of
    the oracle's, an f32 sum of F terms of magnitude <= M in any order plus one division adds less than F x 2^-24 x M
    (tests/test_fbank_tiny_clips.py::test_tiny_uniform_split)."""
    fb = gpu.Fbank()
    noise = np.stack([s16_noise(c, 16000) for c in range(8)])
    clips = [s16_speech(jfk, 0, jfk.shape[0])] + list(noise)
    lens = [c.shape[0] for c in clips]
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    assert frames[0] == 1098
    flat = np.full(n_samples, 12345, np.int16)
    for o, c in zip(offs, clips):
        flat[int(o):int(o) + c.shape[0]] = c
    rows, means = ragged_call(gpu, fb, flat, offs, lens, frames, oo, total, gaps, PCM_S16, out, "io")
    oc = oracle.fbank_default_config()
    oc.apply_cmn = 0
    wants = [oracle.fbank_compute(to_f32(clips[0]), oc)] + list(oracle.fbank_batch(to_f32(noise), oc, THREADS))
    cur = 0
    for c, want in enumerate(wants):
        assert want.shape == (frames[c], NM)
        g = to_f64(rows[cur:cur + want.size], out).reshape(want.shape)
        cur += want.size
        d = np.abs(g - want.astype(np.float64))
        d[np.isnan(d)] = np.inf
        w64 = want.astype(np.float64)
        dm = np.abs(means[c].view(np.float32).astype(np.float64) - w64.mean(axis=0))
        dm[np.isnan(dm)] = np.inf
        bound = TOL + frames[c] * 2.0 ** -24 * float(np.abs(w64).max())
        print(f"FBANK-SPLIT-IO-ORACLE out={out} clip {c}: rows worst {d.max():.3e} (gate {TOL:.1e} + half ulp <= {half_ulp(want, out).max():.3e}), "
              f"means worst {dm.max():.3e} (bound {bound:.3e})")
        assert (d - (TOL + half_ulp(want, out))).max() <= 0.0, (c, float(d.max()))
        assert dm.max() <= bound, (c, float(dm.max()), bound)
    fb.close()


def _calls(gpu, fb, d_pcm, pcm, n, rows_ptr, out, means_ptr, host_src, host_rows, host_means):
    """the three _split_io calls on one clip of n samples -> their statuses"""
    lib = gpu._lib.lib()
    u64p = C.POINTER(C.c_uint64)
    one, ln = np.array([0], np.uint64), np.array([n], np.uint64)
    got = C.c_size_t(77)
    return [lib.melspec_fbank_compute_uniform_device_split_io(fb._h, C.c_void_p(d_pcm), pcm, n, n, 1, C.c_void_p(rows_ptr), out, C.c_void_p(means_ptr), None),
            lib.melspec_fbank_compute_ragged_device_split_io(fb._h, C.c_void_p(d_pcm), pcm, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1, C.c_void_p(rows_ptr), out,
                                                             None, C.c_void_p(means_ptr), None),
            lib.melspec_fbank_compute_host_split_io(fb._h, host_src.ctypes.data_as(C.c_void_p), pcm, n, host_rows.ctypes.data_as(C.c_void_p), out, host_rows.size,
                                                    host_means.ctypes.data_as(C.POINTER(C.c_float)), C.byref(got))]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["40-bins", "magnitudes", "use-generic"])
def test_unsupported_objects_touch_nothing(gpu, case):
    """6a. another bank, magnitude spectra and an object after use_generic: supports_split_io == 0 for every pair, the five combinations
    return MELSPEC_ERR_UNSUPPORTED from the three calls with the geometry in the message, and rows and means -- device and host -- keep
    their sentinels; (F32, F32) is handed to the f32 split calls and runs"""
    lib = gpu._lib.lib()
    kw = {"40-bins": dict(num_mel_bins=40), "magnitudes": dict(use_power=False), "use-generic": {}}[case]
    fb = gpu.Fbank(gpu.FbankConfig(**kw))
    if case == "use-generic":
        assert all(gpu.fbank_supports_split_io(fb, pcm, out) for pcm, out in ALL_COMBOS)
        fb.use_generic(True)
    nm, n = fb.num_mel_bins, 16000
    x = s16_noise(2, n)
    nf = fb.num_frames(n)
    d16 = _upload(gpu, x)
    rows, means = Fence(gpu, nf * nm, OUT_F16), Fence(gpu, nm, OUT_F32)
    for pcm, out in ALL_COMBOS:
        assert not gpu.fbank_supports_split_io(fb, pcm, out)
    for pcm, out in NEW_COMBOS:
        host_rows, host_means = np.full(nf * nm, 0x7DAD, np.uint32), np.full(nm, 777.0, np.float32)
        for rc in _calls(gpu, fb, d16.ptr, pcm, n, rows.ptr, out, means.ptr, x, host_rows, host_means):
            assert rc == ERR_UNSUPPORTED
            msg = lib.melspec_last_error().decode()
            assert f"num_mel_bins = {nm}" in msg and f"use_power = {int(fb.config.use_power)}" in msg and "frame_length = 400 samples" in msg, msg
            assert ("melspec_fbank_use_generic" in msg) == (case == "use-generic"), msg
        assert np.all(host_rows == 0x7DAD) and np.all(host_means == 777.0)
        # the object's checks come in front of "nothing to do"
        assert lib.melspec_fbank_compute_uniform_device_split_io(fb._h, None, pcm, n, n, 0, None, out, None, None) == ERR_UNSUPPORTED
    fb.synchronize()
    assert np.all(rows.bits() == rows.s) and np.all(means.bits() == S_MEANS), "a refused call wrote into a buffer"
    # (F32, F32): the f32 split calls, whatever the object
    x32 = to_f32(x)[None, :]
    d32 = _upload(gpu, x32)
    got = []
    for through_io in (False, True):
        r, m = Fence(gpu, nf * nm, OUT_F32), Fence(gpu, nm, OUT_F32)
        if through_io:
            gpu.fbank_compute_uniform_device_split_io(fb, d32.ptr, PCM_F32, n, n, 1, r.ptr, OUT_F32, m.ptr)
        else:
            fb.compute_uniform_device_split(d32.ptr, n, n, 1, r.ptr, m.ptr)
        fb.synchronize()
        got.append((written(r, "rows"), written(m, "means")))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])
    d16.free(); d32.free()
    fb.close()


@pytest.mark.gpu
def test_checks_in_their_order(gpu):
    """6b. NULL object, dtype codes, apply_cmn off, unsupported object, n_clips == 0, NULL tables, no frame at all (the means zeroed when
    given), NULL device pointers / d_means, misaligned pointers -- each reported in front of everything behind it"""
    lib = gpu._lib.lib()
    u64p = C.POINTER(C.c_uint64)
    n = 16000
    x = s16_noise(3, n)
    one, ln, short = np.array([0], np.uint64), np.array([n], np.uint64), np.array([399], np.uint64)
    P = lambda a: a.ctypes.data_as(u64p)
    ok = gpu.Fbank()
    nf = ok.num_frames(n)
    d = _upload(gpu, x)
    rows, means = Fence(gpu, nf * NM, OUT_F16), Fence(gpu, NM, OUT_F32)
    dp, rp, mp = C.c_void_p(d.ptr), C.c_void_p(rows.ptr), C.c_void_p(means.ptr)
    uni = lambda fb, pcm, out, n_clips, p, r, m, length=n: lib.melspec_fbank_compute_uniform_device_split_io(fb._h, p, pcm, length, length, n_clips, r, out, m, None)
    rag = lambda fb, pcm, out, n_clips, o, l, p, r, m: lib.melspec_fbank_compute_ragged_device_split_io(fb._h, p, pcm, o, l, n_clips, r, out, None, m, None)
    rag32 = lambda fb, n_clips, o, l, p, r, m: lib.melspec_fbank_compute_ragged_device_split(fb._h, p, o, l, n_clips, r, None, m, None)
    # 2. the dtype codes, in front of apply_cmn and of the object's support
    off, forty = gpu.Fbank(gpu.FbankConfig(apply_cmn=False)), gpu.Fbank(gpu.FbankConfig(num_mel_bins=40))
    off40 = gpu.Fbank(gpu.FbankConfig(num_mel_bins=40, apply_cmn=False))
    for pcm, out in ((2, OUT_F16), (-1, OUT_F32), (PCM_S16, 3), (PCM_S16, -1)):
        for fb in (ok, off, forty):
            assert not gpu.fbank_supports_split_io(fb, pcm, out)
            assert uni(fb, pcm, out, 1, dp, rp, mp) == ERR_INVALID_ARG and b"dtype must be" in lib.melspec_last_error()
            assert rag(fb, pcm, out, 1, P(one), P(ln), dp, rp, mp) == ERR_INVALID_ARG and b"dtype must be" in lib.melspec_last_error()
            assert lib.melspec_fbank_compute_host_split_io(fb._h, dp, pcm, n, rp, out, 10 ** 6, None, None) == ERR_INVALID_ARG
    # 3. apply_cmn off: INVALID_ARG with the uniform split's message, in front of the object's support and of "nothing to do"
    for fb in (off, off40):
        assert not gpu.fbank_supports_split_io(fb, PCM_S16, OUT_F16)
        for rc in (uni(fb, PCM_S16, OUT_F16, 1, dp, rp, mp), uni(fb, PCM_S16, OUT_F16, 0, None, None, None), rag(fb, PCM_S16, OUT_F16, 1, P(one), P(ln), dp, rp, mp),
                   rag32(fb, 1, P(one), P(ln), dp, rp, mp), rag32(fb, 0, None, None, None, None, None)):
            assert rc == ERR_INVALID_ARG and b"apply_cmn is off" in lib.melspec_last_error()
    # 4. the unsupported object, in front of "nothing to do" (test_unsupported_objects_touch_nothing has the rest)
    assert rag(forty, PCM_S16, OUT_F16, 0, None, None, None, None, None) == ERR_UNSUPPORTED
    # 5. n_clips == 0: OK, whatever else is NULL
    assert uni(ok, PCM_S16, OUT_F16, 0, None, None, None) == 0 and rag(ok, PCM_S16, OUT_F16, 0, None, None, None, None, None) == 0
    assert rag32(ok, 0, None, None, None, None, None) == 0 and rag32(forty, 0, None, None, None, None, None) == 0
    # 6. NULL tables, in front of the pointers
    for o, l in ((None, P(ln)), (P(one), None)):
        assert rag(ok, PCM_S16, OUT_F16, 1, o, l, None, None, None) == ERR_INVALID_ARG and b"offset/length array is NULL" in lib.melspec_last_error()
        assert rag32(ok, 1, o, l, None, None, None) == ERR_INVALID_ARG and b"offset/length array is NULL" in lib.melspec_last_error()
    # 7. no frame at all: OK with NULL pointers; the mean slots are zeroed when d_means is given, nothing else is touched
    assert uni(ok, PCM_S16, OUT_F16, 1, None, None, None, 399) == 0 and rag(ok, PCM_S16, OUT_F16, 1, P(one), P(short), None, None, None) == 0
    assert rag32(ok, 1, P(one), P(short), None, None, None) == 0
    for call in (lambda m: uni(ok, PCM_S16, OUT_F16, 1, None, None, m, 399), lambda m: rag(ok, PCM_S16, OUT_F16, 1, P(one), P(short), None, None, m),
                 lambda m: rag32(ok, 1, P(one), P(short), None, None, m)):
        z = Fence(gpu, NM, OUT_F32)
        assert call(C.c_void_p(z.ptr)) == 0
        ok.synchronize()
        assert not z.bits().any(), "the means of a batch without a frame are not +0.0"
    # 8. NULL device pointers, then NULL d_means
    for p, r, m, msg in ((None, rp, mp, b"device pointer is NULL"), (dp, None, mp, b"device pointer is NULL"), (None, None, None, b"device pointer is NULL"),
                         (dp, rp, None, b"d_means is NULL")):
        assert uni(ok, PCM_S16, OUT_F16, 1, p, r, m) == ERR_INVALID_ARG and msg in lib.melspec_last_error()
        assert rag(ok, PCM_S16, OUT_F16, 1, P(one), P(ln), p, r, m) == ERR_INVALID_ARG and msg in lib.melspec_last_error()
        assert rag32(ok, 1, P(one), P(ln), p, r, m) == ERR_INVALID_ARG and msg in lib.melspec_last_error()
    # 9. a pointer misaligned for its element type: behind every NULL check
    odd = lambda v: C.c_void_p(v.value + 1)
    two = lambda v: C.c_void_p(v.value + 2)
    assert uni(ok, PCM_S16, OUT_F16, 1, odd(dp), rp, mp, n - 1) == ERR_INVALID_ARG and b"not aligned" in lib.melspec_last_error()
    assert uni(ok, PCM_S16, OUT_F16, 1, dp, odd(rp), mp) == ERR_INVALID_ARG and b"not aligned" in lib.melspec_last_error()
    assert uni(ok, PCM_F32, OUT_F16, 1, two(dp), rp, mp, 4000) == ERR_INVALID_ARG and uni(ok, PCM_S16, OUT_F32, 1, dp, two(rp), mp, 4000) == ERR_INVALID_ARG
    assert rag(ok, PCM_S16, OUT_BF16, 1, P(one), P(ln), dp, odd(rp), mp) == ERR_INVALID_ARG and b"not aligned" in lib.melspec_last_error()
    assert uni(ok, PCM_S16, OUT_F16, 1, odd(dp), rp, None, n - 1) == ERR_INVALID_ARG and b"d_means is NULL" in lib.melspec_last_error()
    ok.synchronize()
    assert np.all(rows.bits() == rows.s) and np.all(means.bits() == S_MEANS), "a refused call wrote into a buffer"
    d.free()
    for fb in (ok, off, forty, off40):
        fb.close()


@pytest.mark.gpu
def test_f32_f32_through_split_io_is_the_f32_split(gpu):
    """6c. (F32, F32) through the _split_io calls: the bits of melspec_fbank_compute_uniform_device_split / _ragged_device_split"""
    fb = gpu.Fbank()
    f32 = to_f32(_mixed(3, 5520, base=2))
    want_means = f32_split_uniform(gpu, fb, f32)
    raw = gpu.Fbank(gpu.FbankConfig(apply_cmn=False))
    want_rows = plain_uniform(gpu, raw, f32)
    raw.close()
    rows, means = split_uniform(gpu, fb, f32, PCM_F32, OUT_F32)
    assert np.array_equal(rows, want_rows) and np.array_equal(means, want_means)
    lens = [5520, 561, 0, 880]
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    flat32 = to_f32(ragged_flat(lens, offs, n_samples))
    tabs = (offs, lens, frames, oo, total, gaps)
    a = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "split")
    b = ragged_call(gpu, fb, flat32, *tabs, PCM_F32, OUT_F32, "io")
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    fb.close()


@pytest.mark.gpu
def test_host_call_equals_device_call(gpu):
    """7. melspec_fbank_compute_host_split_io: bit for bit the device call on one clip, for (S16, F16), (F32, BF16) and (F32, F32); a clip
    without a frame: *n_frames == 0, the rows untouched, the means +0.0; rows_capacity_elems too small: MELSPEC_ERR_CAPACITY; and the
    list form (fbank_compute_ragged_split_io) gives the same clips"""
    lib = gpu._lib.lib()
    fb = gpu.Fbank()
    s16 = _mixed(1, 16000, base=1)
    f32 = to_f32(s16)
    for src, pcm, name, out in ((s16, PCM_S16, "f16", OUT_F16), (f32, PCM_F32, "bf16", OUT_BF16), (f32, PCM_F32, None, OUT_F32)):
        rows, means = split_uniform(gpu, fb, src, pcm, out)
        h_rows, h_means = gpu.fbank_compute_split_io(fb, src[0].copy(), name)
        assert h_rows.shape == (98, NM) and np.array_equal(h_rows.view(rows.dtype), rows[0]), (pcm, out)
        assert np.array_equal(h_means.view(np.uint32), means[0]), (pcm, out)
        short = np.ascontiguousarray(src[0, :399])
        buf, hm = np.full(NM, SENTINEL[out], rows.dtype), np.full(NM, 777.0, np.float32)
        got = C.c_size_t(77)
        assert lib.melspec_fbank_compute_host_split_io(fb._h, short.ctypes.data_as(C.c_void_p), pcm, 399, buf.ctypes.data_as(C.c_void_p), out, buf.size,
                                                       hm.ctypes.data_as(C.POINTER(C.c_float)), C.byref(got)) == 0
        assert got.value == 0 and np.all(buf == SENTINEL[out]) and not hm.view(np.uint32).any()
        many = gpu.fbank_compute_ragged_split_io(fb, [src[0], short, src[0, :5520]], name)
        assert np.array_equal(many[0][0], h_rows) and np.array_equal(many[0][1], h_means)
        assert many[1][0].shape == (0, NM) and not many[1][1].view(np.uint32).any() and many[2][0].shape == (33, NM)
    small, hm = np.zeros(16, np.uint16), np.zeros(NM, np.float32)
    assert lib.melspec_fbank_compute_host_split_io(fb._h, s16.ctypes.data_as(C.c_void_p), PCM_S16, 16000, small.ctypes.data_as(C.c_void_p), OUT_F16, small.size,
                                                   hm.ctypes.data_as(C.POINTER(C.c_float)), None) == ERR_CAPACITY
    fb.close()
