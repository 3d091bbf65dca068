"""Kaldi fbank: int16 PCM in, f16 / bf16 features out (melspec_fbank_compute_uniform_device_io / _ragged_device_io / _host_io).

The yardsticks are those of tests/test_io_dtypes.py, exact, so nothing here is tuned:
  * int16 -> f32 is exact: the int16 call must give THE BITS of the existing f32 call on `batch.astype(float32) * float32(2**-15)` (DC
    removal, pre-emphasis and the Povey window are applied to the converted f32 samples, the first-sample patch of src/fbank.rs:172 included);
  * an f16 / bf16 element is the round-to-nearest-even of the f32 element the existing call writes; with apply_cmn the means are those of
    the f32 rows (the fixed tree of CmnTree) and only row - mean is rounded, once;
  * against the oracle the gate is the fused fbank path's existing gate (tests/test_gpu_parity.py: TOL = 1e-4, test_fbank_jfk) plus half a
    unit in the last place of the 16-bit type at each expected element's own magnitude.
The _io calls always run the two-kernel path (the wave-owned kernel, then the CMN); the existing f32 call runs fbank512_clip_kernel on
large uniform batches.  DESIGN section 3 says the two give the same bits; test_across_the_two_f32_paths relies on it.
Every output sits between two guard bands of a NaN-payload sentinel no kernel computes (tests/test_io_dtypes.py: Fence); ragged outputs
start at odd and even elements with odd gaps between the clips, ragged int16 clips at odd and even samples with foreign samples between."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_io_dtypes import (ERR_CAPACITY, ERR_INVALID_ARG, ERR_UNSUPPORTED, GUARD, NEW_COMBOS, OUT_BF16, OUT_F16, OUT_F32, PCM_F32, PCM_S16,
                            SENTINEL, Fence, _upload, round_to, s16_batch, s16_noise, s16_speech, to_f32, to_f64)
from test_blm_io_dtypes import half_ulp, same

TOL = 1e-4                  # tests/test_gpu_parity.py: TOL, the gate of test_fbank_jfk on the fused fbank path against oracle.fbank_compute
NM = 80
FBANK_IO_SYMBOLS = ["melspec_fbank_supports_io", "melspec_fbank_compute_uniform_device_io", "melspec_fbank_compute_ragged_device_io",
                    "melspec_fbank_compute_host_io"]
# frames = (n - 400) / 160 + 1, four frames per wave unit: no frame (0, 399), 1 frame (400, 401, 559), 2 (560, 561), 4 = one whole unit
# (880), 5 (1040), 32 = exactly eight units, one per run of the CMN's tree (5360), 33 (5520), 98 (16000)
EDGE_LENS = [0, 399, 400, 401, 559, 560, 561, 880, 1040, 5360, 5520, 16000]
RAGGED_LENS = EDGE_LENS + [160000, 0, 4321, 12345, 0, 30000]


def fbank(gpu, **kw):
    fb = gpu.Fbank(gpu.FbankConfig(**kw))
    return fb


@functools.lru_cache(maxsize=None)
def _mixed(n_clips, n, base=0):
    """noise / speech (JFK) / tone / extremes in turn (tests/test_io_dtypes.py: s16_batch 'mixed'); made once per shape"""
    from oracle import oracle as O
    jfk = O.load_wav_f32(os.path.join(ROOT, "tests", "golden", "jfk_f32le.wav"))
    a = s16_batch("mixed", jfk, n_clips, n, base=base)
    a.setflags(write=False)
    return a


def run_uniform(gpu, fb, clips, pcm, out, plain=False, keep=None):
    """clips [n_clips, n] int16 / float32 -> bits [n_clips, frames, 80] of the whole fenced output; plain: the existing f32 call.
    keep: only these clips are downloaded (the guard bands always are)."""
    n_clips, n = clips.shape
    nf = fb.num_frames(n)
    d, f = _upload(gpu, clips), Fence(gpu, n_clips * nf * NM, out)
    if plain:
        fb.compute_uniform_device(d.ptr, n, n, n_clips, f.ptr)
    else:
        fb.compute_uniform_device_io(d.ptr, pcm, n, n, n_clips, f.ptr, out)
    fb.synchronize()
    d.free()
    if keep is not None:
        lo = f.buf.download(GUARD, f.dt)
        hi = f.buf.download(GUARD, f.dt, offset_bytes=(GUARD + f.n) * f.es)
        assert np.all(lo == f.s) and np.all(hi == f.s), "write outside the output"
        res = np.stack([f.buf.download(nf * NM, f.dt, offset_bytes=(GUARD + c * nf * NM) * f.es) for c in keep]).reshape(len(keep), nf, NM)
        f.buf.free()
        assert not (res == f.s).any()
        return res
    bits = f.bits()
    left = bits == f.s
    assert not left.any(), f"uniform ({pcm}, {out}): {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    return bits.reshape(n_clips, nf, NM)


def ragged_tables(fb, lens):
    """sample offsets with a gap of 1 or 2 foreign samples in front of every clip (odd and even starts); output offsets in elements:
    odd gaps, so the clips' rows alternate between odd and even element offsets"""
    offs, cur = [], 0
    for c, n in enumerate(lens):
        cur += 1 + (c % 3 == 0)
        offs.append(cur)
        cur += n
    n_samples = cur + 3
    assert any(o & 1 for o, n in zip(offs, lens) if n >= 400) and any(not o & 1 for o, n in zip(offs, lens) if n >= 400)
    frames = [fb.num_frames(n) for n in lens]
    oo, cur, gaps = [], 0, []
    for c, k in enumerate(frames):
        g = 1 + 2 * (c % 4)
        gaps.append((cur, cur + g))
        cur += g
        oo.append(cur)
        cur += k * NM
    assert any(o & 1 for o, k in zip(oo, frames) if k) and any(not o & 1 for o, k in zip(oo, frames) if k)
    return np.array(offs, np.uint64), n_samples, frames, np.array(oo, np.uint64), cur, gaps


def ragged_flat(lens, offs, n_samples):
    flat = np.full(n_samples, 12345, np.int16)          # between the clips: samples no frame may read into its result
    for c, (o, n) in enumerate(zip(offs, lens)):
        flat[int(o):int(o) + n] = _mixed(1, n, base=c)[0]
    return flat


def run_ragged(gpu, fb, flat, offs, lens, frames, oo, total, gaps, pcm, out, packed=False, plain=False):
    """-> the clips' [frames, 80] bits, concatenated; the gaps between the clips must still hold the sentinel.  plain: the existing f32
    call (melspec_fbank_compute_ragged_device), the reference of a ragged batch."""
    if packed:
        oo = np.concatenate([[0], np.cumsum([k * NM for k in frames])[:-1]]).astype(np.uint64)
        total, gaps = int(sum(frames)) * NM, []
    d, f = _upload(gpu, flat), Fence(gpu, total, out)
    if plain:
        assert (pcm, out) == (PCM_F32, OUT_F32)
        fb.compute_ragged_device(d.ptr, offs, np.array(lens, np.uint64), f.ptr, None if packed else oo)
    else:
        fb.compute_ragged_device_io(d.ptr, pcm, offs, np.array(lens, np.uint64), f.ptr, out, None if packed else oo)
    fb.synchronize()
    bits = f.bits()
    d.free()
    for a, b in gaps:
        assert np.all(bits[a:b] == f.s), f"ragged ({pcm}, {out}): the gap [{a}, {b}) between two outputs was written"
    res = []
    for c, k in enumerate(frames):
        piece = bits[int(oo[c]):int(oo[c]) + k * NM]
        assert not (piece == f.s).any(), f"ragged ({pcm}, {out}): clip {c}: {int((piece == f.s).sum())} elements never written"
        res.append(piece)
    return np.concatenate(res) if res else np.zeros(0, f.dt)


def check_all_combos(gpu, fb, s16, what, ragged=None, packed=False, keep=None):
    """(F32, F32) through the _io call == the plain call; (S16, F32) == the plain call on the converted batch; the four 16-bit outputs
    == its rounding.  Returns the plain call's bits."""
    f32 = to_f32(s16)
    if ragged is None:
        run = lambda src, pcm, out, **kw: run_uniform(gpu, fb, src, pcm, out, keep=keep, **kw).reshape(-1)
    else:
        run = lambda src, pcm, out, **kw: run_ragged(gpu, fb, src, *ragged, pcm, out, packed=packed, **kw)
    want32 = run(f32, PCM_F32, OUT_F32, plain=True)
    assert np.array_equal(run(f32, PCM_F32, OUT_F32), want32), f"{what}: (F32, F32) through the _io call is the plain call"
    for pcm, out in NEW_COMBOS:
        same(run(s16 if pcm == PCM_S16 else f32, pcm, out), want32, out, f"{what} ({pcm}, {out})")
    return want32


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("cmn", [True, False], ids=["cmn", "no-cmn"])
def test_uniform_bits_are_the_f32_calls(gpu, cmn):
    """1. uniform batches of every edge length, twelve clips each (three of each kind: noise, speech, tone, extremes): (S16, F32) equals the
    existing call on the converted batch, the four 16-bit outputs equal its rounding; a length without a frame writes nothing."""
    fb = fbank(gpu, apply_cmn=cmn)
    for pcm, out in NEW_COMBOS:
        assert fb.supports_io(pcm, out)
    for n in EDGE_LENS:
        s16 = _mixed(12, n, base=n % 7)
        want = check_all_combos(gpu, fb, s16, f"uniform n={n} cmn={cmn}")
        assert want.size == 12 * fb.num_frames(n) * NM
    fb.close()


def takes_clip_kernel(n_clips, cus):
    """fbank_launch's rule (clip_uniform_ok, mel_spec_amd/csrc/fused512_route.hpp) for a uniform batch of the default object with CMN: at least one clip per CU
    and the last pass over the CUs at least 85 % full.
    A RESTATEMENT, and of a part only: the rule's other conditions (apply_cmn, use_power, eight waves, a 16-byte aligned output whose
    clip stride is a multiple of four elements: Fence's, behind GUARD = 4096 elements) hold for the batches below without being checked here, and nothing observes which kernel the f32 call really ran -- the library has no hook for
    it.  If the rule in fused512_route.hpp changes, this function has to change with it; otherwise test_across_the_two_f32_paths goes on passing
    while it compares the two-kernel path with itself."""
    passes = (n_clips + cus - 1) // cus
    return n_clips >= cus and n_clips * 100 >= passes * cus * 85


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1040, 16000])
@pytest.mark.parametrize("clips", ["320", "cus", "2cus"])
def test_across_the_two_f32_paths(gpu, n, clips):
    """2. CMN on, all five combinations against the existing f32 call on a large uniform batch; the guard bands and 16 clips spread over
    the batch (first and last included) are downloaded.  320 clips are the issue's case.  fbank_launch gives a uniform batch to
    fbank512_clip_kernel only when the last pass over the CUs is at least 85 % full (takes_clip_kernel): 320 clips on 256 CUs are not,
    so that batch compares the two-kernel path with itself; batches of exactly one and two clips per CU do take the clip kernel and are
    the comparison across the two paths."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_clips = {"320": 320, "cus": cus, "2cus": 2 * cus}[clips]
    if clips != "320":
        assert takes_clip_kernel(n_clips, cus)
    print(f"FBANK-IO-PATHS {n_clips} clips x {n} on {cus} CUs: the f32 call takes the clip kernel: {takes_clip_kernel(n_clips, cus)}")
    fb = fbank(gpu)
    keep = sorted(set(np.linspace(0, n_clips - 1, 16).astype(int).tolist()))
    assert keep[0] == 0 and keep[-1] == n_clips - 1
    check_all_combos(gpu, fb, _mixed(n_clips, n), f"{n_clips} x {n}", keep=keep)
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cmn", [True, False], ids=["cmn", "no-cmn"])
def test_ragged_bits_are_the_f32_calls(gpu, cmn):
    """3. the edge lengths plus 10 s, 4321, 12345 and 30000 samples with empty clips in between; int16 clips at odd and even samples with
    foreign samples (12345) between them; outputs at odd and even element offsets with odd gaps, and once more packed (NULL offsets);
    against melspec_fbank_compute_ragged_device on the converted batch."""
    fb = fbank(gpu, apply_cmn=cmn)
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, RAGGED_LENS)
    flat = ragged_flat(RAGGED_LENS, offs, n_samples)
    args = (offs, RAGGED_LENS, frames, oo, total, gaps)
    a = check_all_combos(gpu, fb, flat, f"ragged cmn={cmn}", ragged=args)
    b = check_all_combos(gpu, fb, flat, f"ragged packed cmn={cmn}", ragged=args, packed=True)
    assert np.array_equal(a, b)
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(preemphasis=0.0), dict(use_log_fbank=False), dict(use_power=False), dict(energy_floor=1e-3)],
                         ids=lambda kw: next(iter(kw)))
def test_configurations(gpu, kw):
    """4. every switch of the fused path, one small uniform and one small ragged batch each, all five combinations.  use_log_fbank = 0:
    energies beyond the f16 range must come out as infinities (the rounding of the f32 element)."""
    fb = fbank(gpu, **kw)
    for pcm, out in NEW_COMBOS:
        assert fb.supports_io(pcm, out)
    check_all_combos(gpu, fb, _mixed(8, 2000), f"uniform {kw}")
    if not kw.get("use_log_fbank", True):
        # int16 samples lie in [-1, 1) and their energies inside the f16 range; f32 samples 256 times as large (exact) do not
        big = fbank(gpu, apply_cmn=False, **kw)
        x = to_f32(_mixed(4, 2000)) * np.float32(256.0)
        want = run_uniform(gpu, big, x, PCM_F32, OUT_F32, plain=True)
        assert np.isfinite(want.view(np.float32)).all() and np.isinf(round_to(want, OUT_F16).view(np.float16)).any()
        for out in (OUT_F16, OUT_BF16):
            same(run_uniform(gpu, big, x, PCM_F32, out), want, out, f"beyond the f16 range (F32, {out})")
        big.close()
    lens = [2000, 0, 561, 880, 4321, 399, 1040]
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    check_all_combos(gpu, fb, ragged_flat(lens, offs, n_samples), f"ragged {kw}", ragged=(offs, lens, frames, oo, total, gaps))
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shift_ms, shift", [(12.0, 192), (10.0625, 161)], ids=["192", "161"])
def test_other_frame_shifts(gpu, shift_ms, shift):
    """The frame shift is a run-time value of the kernel and not part of what melspec_fbank_supports_io asks for (the header says so): an
    object with 25 ms frames every 12 ms, and one with an odd shift of 161 samples (every other frame of an int16 clip starts at an odd
    sample), are supported and give the bits of their own f32 calls, CMN on, one small uniform and one small ragged batch."""
    fb = fbank(gpu, frame_shift_ms=shift_ms)
    assert fb.config.frame_shift_samples() == shift and fb.num_frames(2000) == (2000 - 400) // shift + 1
    for pcm, out in NEW_COMBOS:
        assert fb.supports_io(pcm, out)
    check_all_combos(gpu, fb, _mixed(8, 2000), f"uniform shift={shift}")
    lens = [2000, 0, 400 + shift, 400 + 4 * shift - 1, 4321, 399, 400 + 4 * shift]
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    check_all_combos(gpu, fb, ragged_flat(lens, offs, n_samples), f"ragged shift={shift}", ragged=(offs, lens, frames, oo, total, gaps))
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
def test_s16_in_16bit_out_against_the_oracle(gpu, oracle, jfk, out):
    """5. the JFK clip whole (1098 frames) and eight noise clips of 1 s in one ragged batch, (S16, 16-bit), CMN on, against oracle.fbank_compute
    on the exactly converted samples.  Bound per element = the fused fbank path's existing gate (tests/test_gpu_parity.py: TOL = 1e-4,
    test_fbank_jfk / test_fbank_ragged_batches) + half a unit in the last place of the 16-bit type at the expected element's magnitude."""
    fb = fbank(gpu)
    clips = [s16_speech(jfk, 0, jfk.shape[0])] + [s16_noise(c, 16000) for c in range(8)]
    lens = [c.shape[0] for c in clips]
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    assert frames[0] == 1098
    flat = np.full(n_samples, 12345, np.int16)
    for o, c in zip(offs, clips):
        flat[int(o):int(o) + c.shape[0]] = c
    got = run_ragged(gpu, fb, flat, offs, lens, frames, oo, total, gaps, PCM_S16, out)
    cur = 0
    for c, x in enumerate(clips):
        want = oracle.fbank_compute(to_f32(x))
        assert want.shape == (frames[c], NM)
        g = to_f64(got[cur:cur + want.size], out).reshape(want.shape)
        cur += want.size
        d = np.abs(g - want.astype(np.float64))
        d[np.isnan(d)] = np.inf
        print(f"FBANK-IO-ORACLE out={out} clip {c}: worst {d.max():.3e}, gate {TOL:.1e} + half ulp <= {half_ulp(want, out).max():.3e}")
        assert (d - (TOL + half_ulp(want, out))).max() <= 0.0, (c, float(d.max()))
    fb.close()


@pytest.mark.gpu
def test_host_call_equals_device_call(gpu):
    """6. melspec_fbank_compute_host_io, bit for bit the device call, for (S16, F16) and (F32, BF16) on a 1 s clip; a 399-sample clip has no
    frame: *n_frames == 0 and the output is untouched."""
    lib = gpu._lib.lib()
    fb = fbank(gpu)
    s16 = _mixed(1, 16000, base=1)
    f32 = to_f32(s16)
    for src, pcm, name, out in ((s16, PCM_S16, "f16", OUT_F16), (f32, PCM_F32, "bf16", OUT_BF16)):
        dev = run_uniform(gpu, fb, src, pcm, out)[0]
        host = fb.compute_host_io(src[0].copy(), name)
        assert host.shape == (98, NM) and np.array_equal(host.view(np.uint16), dev), (pcm, out)
        short = np.ascontiguousarray(src[0, :399])
        buf = np.full(NM, SENTINEL[out], np.uint16)
        got = C.c_size_t(77)
        assert lib.melspec_fbank_compute_host_io(fb._h, short.ctypes.data_as(C.c_void_p), pcm, 399, buf.ctypes.data_as(C.c_void_p), out, buf.size, C.byref(got)) == 0
        assert got.value == 0 and np.all(buf == SENTINEL[out])
        assert fb.compute_host_io(short, name).shape == (0, NM)
    small = np.zeros(16, np.uint16)
    assert lib.melspec_fbank_compute_host_io(fb._h, s16.ctypes.data_as(C.c_void_p), PCM_S16, 16000, small.ctypes.data_as(C.c_void_p), OUT_F16, small.size, None) == ERR_CAPACITY
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["40-bins", "22050-hz", "use-generic"])
def test_unsupported_objects_and_bad_arguments(gpu, case):
    """7. another bank, another geometry and an object after use_generic(True): supports_io == 0 for the five new combinations and 1 for
    (F32, F32), the three calls return MELSPEC_ERR_UNSUPPORTED with the geometry in the message, the fenced output stays all sentinel;
    (F32, F32) through the _io calls equals the plain calls.  On a supported object: unknown dtype codes, NULL and misaligned pointers
    are MELSPEC_ERR_INVALID_ARG."""
    lib = gpu._lib.lib()
    u64p = C.POINTER(C.c_uint64)
    kw = {"40-bins": dict(num_mel_bins=40), "22050-hz": dict(sample_rate=22050.0), "use-generic": {}}[case]
    fb = fbank(gpu, **kw)
    if case == "use-generic":
        for pcm, out in NEW_COMBOS:
            assert fb.supports_io(pcm, out)
        fb.use_generic(True)
    nm, n = fb.num_mel_bins, 16000
    x = s16_noise(2, n)
    nf = fb.num_frames(n)
    d16 = _upload(gpu, x)
    f = Fence(gpu, nf * nm, OUT_F16)
    one, ln = np.array([0], np.uint64), np.array([n], np.uint64)
    assert fb.supports_io(PCM_F32, OUT_F32)
    for pcm, out in NEW_COMBOS:
        assert not fb.supports_io(pcm, out)
        assert lib.melspec_fbank_compute_uniform_device_io(fb._h, C.c_void_p(d16.ptr), pcm, n, n, 1, C.c_void_p(f.ptr), out, None) == ERR_UNSUPPORTED
        msg = lib.melspec_last_error().decode()
        assert f"num_mel_bins = {nm}" in msg and f"sample_rate = {fb.config.sample_rate:g}" in msg and \
            f"frame_length = {fb.config.frame_length_samples()} samples" in msg, msg
        assert ("melspec_fbank_use_generic" in msg) == (case == "use-generic"), msg
        assert lib.melspec_fbank_compute_ragged_device_io(fb._h, C.c_void_p(d16.ptr), pcm, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1,
                                                          C.c_void_p(f.ptr), out, None, None) == ERR_UNSUPPORTED
        host_out = np.full(nf * nm, 0x7DAD, np.uint16)
        got = C.c_size_t(77)
        assert lib.melspec_fbank_compute_host_io(fb._h, x.ctypes.data_as(C.c_void_p), pcm, n, host_out.ctypes.data_as(C.c_void_p), out, host_out.size,
                                                 C.byref(got)) == ERR_UNSUPPORTED
        assert np.all(host_out == 0x7DAD)
    fb.synchronize()
    assert np.all(f.bits() == np.uint16(SENTINEL[OUT_F16])), "a refused call wrote into the output"
    # (F32, F32) through the _io entry points: the existing calls
    x32 = to_f32(x)
    d32 = _upload(gpu, x32)
    fa, fb_ = Fence(gpu, nf * nm, OUT_F32), Fence(gpu, nf * nm, OUT_F32)
    fb.compute_uniform_device(d32.ptr, n, n, 1, fa.ptr)
    fb.compute_uniform_device_io(d32.ptr, PCM_F32, n, n, 1, fb_.ptr, OUT_F32)
    fb.synchronize()
    plain = fa.bits()
    assert not (plain == fa.s).any() and np.array_equal(plain, fb_.bits())
    fa, fb_ = Fence(gpu, nf * nm, OUT_F32), Fence(gpu, nf * nm, OUT_F32)
    fb.compute_ragged_device(d32.ptr, one, ln, fa.ptr)
    fb.compute_ragged_device_io(d32.ptr, PCM_F32, one, ln, fb_.ptr, OUT_F32)
    fb.synchronize()
    assert np.array_equal(fa.bits(), plain) and np.array_equal(fb_.bits(), plain)
    assert np.array_equal(fb.compute_host_io(x32).view(np.uint32).reshape(-1), fb.compute(x32).view(np.uint32).reshape(-1))
    d16.free(); d32.free()
    fb.close()
    if case != "40-bins":
        return
    ok = fbank(gpu)
    f = Fence(gpu, ok.num_frames(n) * NM, OUT_F16)
    d = _upload(gpu, x)
    for pcm, out in ((2, OUT_F16), (-1, OUT_F32), (PCM_S16, 3), (PCM_S16, -1)):
        assert not ok.supports_io(pcm, out)
        assert lib.melspec_fbank_compute_uniform_device_io(ok._h, C.c_void_p(d.ptr), pcm, n, n, 1, C.c_void_p(f.ptr), out, None) == ERR_INVALID_ARG
        assert lib.melspec_fbank_compute_ragged_device_io(ok._h, C.c_void_p(d.ptr), pcm, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1,
                                                          C.c_void_p(f.ptr), out, None, None) == ERR_INVALID_ARG
        assert lib.melspec_fbank_compute_host_io(ok._h, x.ctypes.data_as(C.c_void_p), pcm, n, x.ctypes.data_as(C.c_void_p), out, 10 ** 6, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_uniform_device_io(ok._h, None, PCM_S16, n, n, 1, C.c_void_p(f.ptr), OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_uniform_device_io(ok._h, C.c_void_p(d.ptr), PCM_S16, n, n, 1, None, OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_uniform_device_io(ok._h, C.c_void_p(d.ptr + 1), PCM_S16, n - 1, n - 1, 1, C.c_void_p(f.ptr), OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_uniform_device_io(ok._h, C.c_void_p(d.ptr), PCM_S16, n, n, 1, C.c_void_p(f.ptr + 1), OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_ragged_device_io(ok._h, C.c_void_p(d.ptr), PCM_S16, None, ln.ctypes.data_as(u64p), 1, C.c_void_p(f.ptr), OUT_F16, None, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_ragged_device_io(ok._h, None, PCM_S16, one.ctypes.data_as(u64p), ln.ctypes.data_as(u64p), 1, C.c_void_p(f.ptr), OUT_F16, None, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_host_io(ok._h, None, PCM_S16, n, x.ctypes.data_as(C.c_void_p), OUT_F16, 10 ** 6, None) == ERR_INVALID_ARG
    ok.synchronize()
    assert np.all(f.bits() == np.uint16(SENTINEL[OUT_F16]))
    d.free()
    ok.close()


@pytest.mark.gpu
def test_scratch_and_stream_hand_over(gpu):
    """8. a 16-bit CMN call, melspec_fbank_release_scratch, the same call again: the same bits.  Then a call on a caller stream followed by
    one of another shape on the object's own stream, read after both: the second call's use of the scratch waits for the first's."""
    fb = fbank(gpu)
    a, b = _mixed(40, 48160, base=3), _mixed(9, 8000, base=50)
    want_a = run_uniform(gpu, fb, to_f32(a), PCM_F32, OUT_F32, plain=True)
    want_b = run_uniform(gpu, fb, to_f32(b), PCM_F32, OUT_F32, plain=True)
    first = run_uniform(gpu, fb, a, PCM_S16, OUT_BF16)
    same(first, want_a, OUT_BF16, "before release_scratch")
    fb.release_scratch()
    assert np.array_equal(run_uniform(gpu, fb, a, PCM_S16, OUT_BF16), first), "after release_scratch"
    # ragged, with offsets of the caller's behind the rows in the scratch
    lens = [4321, 0, 16000, 880]
    offs, n_samples, frames, oo, total, gaps = ragged_tables(fb, lens)
    flat = ragged_flat(lens, offs, n_samples)
    args = (offs, lens, frames, oo, total, gaps)
    want_r = run_ragged(gpu, fb, to_f32(flat), *args, PCM_F32, OUT_F32, plain=True)
    same(run_ragged(gpu, fb, flat, *args, PCM_S16, OUT_F16), want_r, OUT_F16, "ragged after the scratch shrank")
    other = torch.cuda.Stream()
    da, db = _upload(gpu, a), _upload(gpu, b)
    fa, fb_ = Fence(gpu, want_a.size, OUT_F16), Fence(gpu, want_b.size, OUT_F16)
    torch.cuda.synchronize()
    fb.compute_uniform_device_io(da.ptr, PCM_S16, a.shape[1], a.shape[1], a.shape[0], fa.ptr, OUT_F16, stream=other.cuda_stream)
    fb.compute_uniform_device_io(db.ptr, PCM_S16, b.shape[1], b.shape[1], b.shape[0], fb_.ptr, OUT_F16)
    fb.synchronize()
    other.synchronize()
    same(fa.bits(), want_a, OUT_F16, "the call on the caller's stream")
    same(fb_.bits(), want_b, OUT_F16, "the call on the object's stream behind it")
    da.free(); db.free()
    fb.close()


CPP_MIRROR = r"""
#include "melspec_hip.hpp"
#include <cstdio>
int main(int argc, char **argv) {
    melspec::Fbank fb;
    if (!fb.supports_io(MELSPEC_PCM_S16, MELSPEC_OUT_F16) || !fb.supports_io(MELSPEC_PCM_S16, MELSPEC_OUT_BF16)) return 2;
    std::vector<std::int16_t> x(16000);
    for (int i = 0; i < 16000; ++i) x[i] = static_cast<std::int16_t>((i * 7919) % 65536 - 32768);
    std::size_t frames = 0;
    const std::vector<std::uint16_t> a = fb.compute_s16(x, MELSPEC_OUT_F16, &frames);
    if (frames != 98 || a.size() != 98 * 80) return 3;
    fb.synchronize();
    fb.release_scratch();
    const std::vector<std::uint16_t> b = fb.compute_s16(x, MELSPEC_OUT_BF16, &frames);
    if (frames != 98 || b.size() != 98 * 80) return 4;
    // the device members are only compiled here (tests/test_fbank_io_dtypes.py runs the C calls behind them): no clip, no launch
    fb.compute_uniform_device_io(nullptr, MELSPEC_PCM_S16, 0, 0, 0, nullptr, MELSPEC_OUT_F16);
    fb.compute_ragged_device_io(nullptr, MELSPEC_PCM_S16, {}, {}, nullptr, MELSPEC_OUT_F16);
    std::FILE *f = std::fopen(argv[1], "wb");
    if (!f || std::fwrite(a.data(), 2, a.size(), f) != a.size() || std::fwrite(b.data(), 2, b.size(), f) != b.size() || std::fclose(f)) return 5;
    std::puts("OK");
    return 0;
}
"""


@pytest.mark.gpu
def test_cpp_mirror(gpu, tmp_path):
    """include/melspec_hip.hpp: Fbank::supports_io, compute_s16, synchronize and release_scratch run, the two device members compile and
    return on an empty batch; compute_s16's bits are those of the Python mirror's compute_host_io on the same samples.  (Built and run
    like tests/test_gpu_parity.py: test_cpp_host_mirror.)"""
    import subprocess
    src, exe, res = tmp_path / "fbank_io_mirror.cpp", tmp_path / "fbank_io_mirror", tmp_path / "rows.bin"
    src.write_text(CPP_MIRROR)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-L", os.path.join(ROOT, "mel_spec_amd"),
                           "-lmelspec_hip", "-Wl,-rpath," + os.path.join(ROOT, "mel_spec_amd"), "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)])
    p = subprocess.run([str(exe), str(res)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip().endswith("OK"), p.stdout + p.stderr
    got = np.fromfile(res, np.uint16).reshape(2, 98, NM)
    x = ((np.arange(16000, dtype=np.int64) * 7919) % 65536 - 32768).astype(np.int16)
    fb = fbank(gpu)
    assert np.array_equal(got[0], fb.compute_host_io(x, "f16").view(np.uint16))
    assert np.array_equal(got[1], fb.compute_host_io(x, "bf16").view(np.uint16))
    fb.close()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_fbank_io_symbols_everywhere():
    """the four entry points resolve in the built library and are declared in the header, the ctypes table and the Rust shim"""
    from mel_spec_amd import _lib
    lib = _lib.lib()
    header = open(os.path.join(ROOT, "include", "melspec_hip.h")).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    for name in FBANK_IO_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f'"{name}"' in table, name
        assert re.search(rf"\bfn {name}\s*\(", shim), name
    assert lib.melspec_abi_version() == 1


def test_fbank_io_null_object_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.int16)
    p = buf.ctypes.data_as(C.c_void_p)
    for pcm, out in NEW_COMBOS + [(PCM_F32, OUT_F32)]:
        assert lib.melspec_fbank_supports_io(None, pcm, out) == 0
    assert lib.melspec_fbank_compute_uniform_device_io(None, p, PCM_S16, 1024, 1024, 1, p, OUT_F16, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_ragged_device_io(None, p, PCM_S16, None, None, 1, p, OUT_F16, None, None) == ERR_INVALID_ARG
    assert lib.melspec_fbank_compute_host_io(None, p, PCM_S16, 1024, p, OUT_F16, 1024, None) == ERR_INVALID_ARG
    assert b"fbank is NULL" in lib.melspec_last_error()


def test_python_mirror_has_the_four_methods():
    import mel_spec_amd as M
    for name in ("supports_io", "compute_uniform_device_io", "compute_ragged_device_io", "compute_host_io"):
        assert callable(getattr(M.Fbank, name)), name
