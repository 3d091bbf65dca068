"""NeMo / Parakeet frontend: the split output (melspec_blm_compute_uniform_device_split / _host_split / melspec_blm_supports_split) --
the un-normalised log-mel rows plus, per (clip, mel) row, the mean and 1 / (std + 1e-5) of normalize_per_feature (src/mel.rs:721-749),
accumulated by the mel kernel itself instead of a second pass over the rows.

What is checked, and against what:
  * the rows are THE BITS of melspec_blm_compute_uniform_device from a context with normalize_per_feature = 0 in the same precision mode;
  * mean / inv_std against numpy f64 statistics of the rows the call returned: |mean - mean64| <= 1e-5 max|row|, inv_std within 1e-5
    relative (f32 partials over at most 48 values, 48 * 2^-24 ~ 3e-6, merged in f64; a factor of three of slack), at the clip lengths
    where a block, a unit or a row ends: 1, 2, 4, 5, 31, 32, 33, 47, 48, 49, 97 and 1001 valid frames;
  * (rows - mean) * inv_std against the oracle's normalised output with tests/test_gpu_parity.py's numbers (_check_nemo_normalised: rows
    whose f64 std is >= 0.5, 1e-4 relative to max(1, |z|)); ill-conditioned rows are not gated against the oracle's f32 left fold, which
    these statistics are more accurate than by design;
  * the statistics of a clip are the same bits wherever the clip sits in whatever batch, and from run to run;
  * contexts without the kernels return MELSPEC_ERR_UNSUPPORTED and touch nothing; a clip length without a frame returns OK and writes nothing.
Every output buffer sits between two guard bands of a NaN-payload sentinel no kernel computes (tests/test_io_dtypes.py: Fence)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_io_dtypes import ERR_INVALID_ARG, ERR_UNSUPPORTED, OUT_F32, Fence, _upload

TOL = 1e-4                  # tests/test_gpu_parity.py
SPLIT_SYMBOLS = ["melspec_blm_supports_split", "melspec_blm_compute_uniform_device_split", "melspec_blm_compute_host_split"]
VALID_FRAMES = [1, 2, 4, 5, 31, 32, 33, 47, 48, 49, 97, 1001]


def frontend(gpu, nm, mode="f64", **kw):
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(n_mels=nm, **kw))
    fe.set_precision(mode)
    if kw.get("n_fft", 512) == 512 and kw.get("win_length", 400) == 400 and nm in (80, 128):
        assert fe.precision == mode
    return fe


def noise(seed, shape, scale=0.1):
    return (np.random.default_rng(seed).standard_normal(shape) * scale).astype(np.float32)


def f32(bits):
    return np.ascontiguousarray(bits).view(np.float32)


def run_split(gpu, fe, clips, expect_written=True):
    """clips [n_clips, n] float32 -> bits (rows [n_clips, n_mels, cols], mean [n_clips, n_mels], inv_std [n_clips, n_mels]) of the three
    fenced outputs; expect_written=False: the call must leave all three as they were"""
    n_clips, n = clips.shape
    nm, cols = fe.config.n_mels, fe.padded_frames(n)
    d = _upload(gpu, clips)
    fr, fm, fs = Fence(gpu, n_clips * nm * max(cols, 1), OUT_F32), Fence(gpu, n_clips * nm, OUT_F32), Fence(gpu, n_clips * nm, OUT_F32)
    rc = gpu._lib.lib().melspec_blm_compute_uniform_device_split(fe._h, C.c_void_p(d.ptr), n, n, n_clips, C.c_void_p(fr.ptr), C.c_void_p(fm.ptr),
                                                                C.c_void_p(fs.ptr), None)
    fe.synchronize()
    rows, mean, inv_std = fr.bits(), fm.bits(), fs.bits()          # (checks the guard bands)
    d.free()
    if not expect_written:
        assert np.all(rows == fr.s) and np.all(mean == fm.s) and np.all(inv_std == fs.s), "a call that computes nothing wrote to its outputs"
        return rc
    assert rc == 0, gpu._lib.lib().melspec_last_error()
    for name, b, f in (("rows", rows, fr), ("mean", mean, fm), ("inv_std", inv_std, fs)):
        left = b == f.s
        assert not left.any(), f"{name}: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    return rows.reshape(n_clips, nm, cols), mean.reshape(n_clips, nm), inv_std.reshape(n_clips, nm)


def run_raw(gpu, fe, clips):
    n_clips, n = clips.shape
    nm, cols = fe.config.n_mels, fe.padded_frames(n)
    d, f = _upload(gpu, clips), Fence(gpu, n_clips * nm * cols, OUT_F32)
    fe.compute_uniform_device(d.ptr, n, n, n_clips, f.ptr)
    fe.synchronize()
    bits = f.bits()
    d.free()
    return bits.reshape(n_clips, nm, cols)


def stats64(rows, valid):
    x = rows[..., :valid].astype(np.float64)
    mean = x.mean(axis=-1)
    var = ((x - mean[..., None]) ** 2).sum(axis=-1) / max(valid - 1, 1)
    return mean, 1.0 / (np.sqrt(var) + 1e-5)


def check_stats(rows, mean, inv_std, valid, what):
    """Test 2's margins against the f64 statistics of the returned rows; prints the figures before it asserts"""
    m64, s64 = stats64(rows, valid)
    peak = np.abs(rows[..., :valid]).max(axis=-1)
    dm = float((np.abs(mean.astype(np.float64) - m64) / peak).max())
    ds = float((np.abs(inv_std.astype(np.float64) - s64) / s64).max())
    print(f"{what}: |mean - mean64| / max|row| = {dm:.3e}, inv_std relative = {ds:.3e}")
    assert dm <= 1e-5, (what, dm)
    assert ds <= 1e-5, (what, ds)


# ---- Test 1: the rows are the raw call's bits ------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("pad_to", [0, 16])
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_rows_are_the_raw_calls_bits(gpu, oracle, nm, mode, pad_to, center):
    kw = dict(pad_to=pad_to, center=center, preemphasis=0.97)
    clips = np.stack([oracle.synth_pcm(c, 16007) for c in range(5)])          # 101 / 97 valid frames: blocks and units end inside the row
    raw_fe = frontend(gpu, nm, mode, normalize_per_feature=False, **kw)
    want = run_raw(gpu, raw_fe, clips)
    valid, cols = raw_fe.num_frames(16007), raw_fe.padded_frames(16007)
    raw_fe.close()
    assert np.all(want[:, :, valid:] == 0), "pad columns of the raw call"
    for norm in (False, True):                           # the context's own normalize_per_feature does not matter to the call
        fe = frontend(gpu, nm, mode, normalize_per_feature=norm, **kw)
        assert fe.supports_split()
        rows, mean, inv_std = run_split(gpu, fe, clips)
        fe.close()
        assert rows.shape == (5, nm, cols)
        diff = rows != want
        assert not diff.any(), f"{int(diff.sum())} row elements differ from the raw call (first at {np.argwhere(diff)[0]})"
        assert np.all(rows[:, :, valid:] == 0), "pad columns are +0"
        check_stats(f32(rows), f32(mean), f32(inv_std), valid, f"{nm} {mode} pad_to {pad_to} center {center}")


# ---- Test 2: the statistics against f64 ----------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_statistics_against_f64(gpu, oracle, nm, mode):
    fe = frontend(gpu, nm, mode)
    for valid in VALID_FRAMES:
        n = (valid - 1) * 160 + (100 if valid == 1 else 0)            # center: valid = n / 160 + 1
        assert fe.num_frames(n) == valid
        clips = np.stack([oracle.synth_pcm(10 * valid + c, n) for c in range(3)])
        rows, mean, inv_std = run_split(gpu, fe, clips)
        rows, mean, inv_std = f32(rows), f32(mean), f32(inv_std)
        assert np.isfinite(rows).all() and np.isfinite(mean).all() and np.isfinite(inv_std).all()
        if valid == 1:                                  # var = 0: mean = the value, inv_std = 1 / 1e-5, as in the reference
            assert np.array_equal(mean, rows[:, :, 0]) and np.all(inv_std == np.float32(1e5)), (mean[0, :4], inv_std[0, :4])
        check_stats(rows, mean, inv_std, valid, f"{nm} {mode} {valid} frames")
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_constant_rows_have_no_deviation(gpu, mode):
    """Digital silence: every row is one value repeated.  A plain f32 sum of 48 equal values already rounds, and merged block means that
    differ in the last place come out as a standard deviation; built as first value + mean distance, the partials are exact here."""
    fe = frontend(gpu, 128, mode)
    rows, mean, inv_std = run_split(gpu, fe, np.zeros((2, 16000), np.float32))
    fe.close()
    rows, mean, inv_std = f32(rows), f32(mean), f32(inv_std)
    assert np.all(rows == rows[:, :, :1])
    assert np.array_equal(mean, rows[:, :, 0]) and np.all(inv_std == np.float32(1e5))


# ---- Test 3: the contract end to end -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(n_mels=128, preemphasis=0.97)])
def test_normalised_by_the_consumer_matches_the_oracle(gpu, oracle, jfk, kw):
    """(rows - mean) * inv_std on the valid columns against the oracle's normalize_per_feature output, with the numbers
    tests/test_gpu_parity.py (_check_nemo_normalised) applies to the fused call: the un-normalised rows within 1e-4, and on the rows whose
    f64 std is >= 0.5 the normalised values within 1e-4 relative to max(1, |z|)."""
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    cfg_raw = oracle.blm_default_config(**kw)
    cfg_norm = oracle.blm_default_config(normalize_per_feature=1, **kw)
    gated = 0
    for x in (jfk, oracle.synth_pcm(2, 16007), oracle.synth_pcm(5, 48000)):
        rows, mean, inv_std = fe.compute_split(x)
        raw_want, valid = oracle.blm_compute(x, cfg_raw, True)
        want, _ = oracle.blm_compute(x, cfg_norm, True)
        assert rows.shape == want.shape and fe.num_frames(len(x)) == valid
        assert np.abs(rows - raw_want).max() <= TOL
        got = np.zeros_like(rows)
        got[:, :valid] = (rows[:, :valid] - mean[:, None]) * inv_std[:, None]
        std = raw_want[:, :valid].astype(np.float64).std(axis=1, ddof=1)
        good = std >= 0.5
        assert good.any()
        d = np.abs(got[good] - want[good]) / np.maximum(1.0, np.abs(want[good]))
        print(f"{kw} {len(x)} samples: {int(good.sum())} rows gated, worst {float(d.max()):.3e}")
        assert d.max() <= TOL, float(d.max())
        gated += int(good.sum())
    fe.close()
    assert gated > 0


# ---- Test 4: a clip's statistics do not depend on where it is ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_position_independence(gpu, oracle, nm, mode):
    """One clip's content first, in the middle and last in batches of 1, 7 and 600 clips of 0.5 s and of 3 and 40 clips of 10 s (the large
    batches run past one trip of the grid: a workgroup sees many rounds, most of them of other clips): mean and inv_std are the same
    bits in every placement, and the same batch run twice gives the same bits."""
    fe = frontend(gpu, nm, mode, pad_to=16 if nm == 80 else 0)
    for n, sizes in ((8000, (1, 7, 600)), (160000, (3, 40))):
        probe = oracle.synth_pcm(77, n)
        ref = None
        for size in sizes:
            filler = noise(size, (size, n))
            for at in sorted({0, size // 2, size - 1}):
                clips = filler.copy()
                clips[at] = probe
                rows, mean, inv_std = run_split(gpu, fe, clips)
                got = (rows[at].copy(), mean[at].copy(), inv_std[at].copy())
                if ref is None:
                    ref = got
                    check_stats(f32(rows[at]), f32(mean[at]), f32(inv_std[at]), fe.num_frames(n), f"{nm} {mode} {n} samples")
                for name, a, b in zip(("rows", "mean", "inv_std"), got, ref):
                    assert np.array_equal(a, b), f"{name} of the clip at {at} of {size} x {n} samples differ from the first placement in {int((a != b).sum())} elements"
            again = run_split(gpu, fe, clips)
            for name, a, b in zip(("rows", "mean", "inv_std"), again, (rows, mean, inv_std)):
                assert np.array_equal(a, b), f"{name}: the same batch of {size} clips gave other bits the second time"
    fe.close()


# ---- Test 5: what is supported ------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_supports_split_and_unsupported_contexts(gpu, oracle):
    clips = np.stack([oracle.synth_pcm(c, 4000) for c in range(2)])
    for kw in (dict(n_mels=40), dict(n_mels=80, n_fft=1024, win_length=800, hop_length=256), dict(n_mels=80, n_fft=512, win_length=320)):
        fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
        assert not fe.supports_split(), kw
        assert run_split(gpu, fe, clips, expect_written=False) == ERR_UNSUPPORTED
        msg = gpu._lib.lib().melspec_last_error().decode()
        assert "split output" in msg and f"n_mels = {kw['n_mels']}" in msg and f"n_fft = {kw.get('n_fft', 512)}" in msg, msg
        with pytest.raises(Exception):
            fe.compute_split(clips[0])
        fe.close()
    for nm in (80, 128):
        for mode in ("f64", "f32"):
            fe = frontend(gpu, nm, mode, center=False)
            assert fe.supports_split()
            # no frame: center = False and fewer samples than n_fft -> OK, nothing written
            assert fe.num_frames(300) == 0
            assert run_split(gpu, fe, np.stack([oracle.synth_pcm(c, 300) for c in range(3)]), expect_written=False) == 0
            rows, mean, inv_std = fe.compute_split(oracle.synth_pcm(1, 300))
            assert rows.shape == (nm, 0)
            fe.close()


# ---- Test 6: the host form ----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_host_form_is_the_device_call(gpu, oracle, nm, mode):
    fe = frontend(gpu, nm, mode, pad_to=16)
    x = oracle.synth_pcm(9, 16007)
    rows, mean, inv_std = fe.compute_split(x)
    d_rows, d_mean, d_inv_std = run_split(gpu, fe, x[None, :])
    fe.close()
    assert np.array_equal(rows.view(np.uint32), d_rows[0]) and np.array_equal(mean.view(np.uint32), d_mean[0]) and np.array_equal(inv_std.view(np.uint32), d_inv_std[0])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_split_symbols_everywhere():
    """the three entry points resolve in the built library and are declared in the header, the ctypes table, the C++ wrapper and the Rust
    shim; the header is still C99"""
    from mel_spec_amd import _lib
    lib = _lib.lib()
    header_path = os.path.join(ROOT, "include", "melspec_hip.h")
    header = open(header_path).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    wrapper = open(os.path.join(ROOT, "include", "melspec_hip.hpp")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    for name in SPLIT_SYMBOLS:
        assert getattr(lib, name) is not None
        assert re.search(rf"\b{name}\s*\(", header), name
        assert f'"{name}"' in table, name
        assert re.search(rf"\b{name}\s*\(", wrapper), name
        assert re.search(rf"\bfn {name}\s*\(", shim), name
    assert "src/mel.rs:721-749" in header
    assert lib.melspec_abi_version() == 1
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-x", "c", header_path])


def test_split_null_context_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    fp = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.melspec_blm_supports_split(None) == 0
    assert lib.melspec_blm_compute_uniform_device_split(None, p, 1024, 1024, 1, p, p, p, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_compute_host_split(None, fp, 1024, fp, 1024, fp, fp, None, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_split_plan_and_arguments_on_the_host(tmp_path, sanitize):
    """the arithmetic half of the host side (mel_spec_amd/csrc/blm_stats_plan.hpp) as a stand-alone program, plain and with
    -fsanitize=address,undefined: tests/cpp/blm_stats_host.cpp"""
    exe = tmp_path / "blm_stats_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blm_stats_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("blm_stats_host: ok"), p.stdout + p.stderr
