"""NeMo / Parakeet frontend: the split output for ragged batches (melspec_blm_compute_ragged_device_split) -- clips of any length in one
launch, each with its un-normalised log-mel rows and the per-feature mean and 1 / (std + 1e-5) of normalize_per_feature.

The yardstick is the EXISTING uniform call, melspec_blm_compute_uniform_device_split (tests/test_blm_split.py: run_split), never the new
code: a clip's rows, mean and inv_std out of a ragged batch have to be the bits that call gives for the clip alone, in the same precision
mode -- whatever the clip's place in the batch, the other clips, the batch's size or the output offsets.  What is checked:
  * the bits, at the clip lengths where a block (32 / 48 frames), a unit (4 frames) or a row ends, with a frameless clip in the middle;
    pad columns +0; the frameless clip's statistics slots untouched; the statistics against numpy f64 with test_blm_split's margins;
  * caller-chosen row offsets (reverse order, gaps): the gaps and the guard bands stay untouched;
  * a batch of 4099 clips, well past one trip of the grid, against one uniform call per distinct length; the same batch twice;
  * constant rows (digital silence): mean == the value, inv_std == 1e5 exactly;
  * the Python entry point against the oracle with tests/test_gpu_parity.py's numbers;
  * the refusals: unsupported contexts, NULL tables, NULL device pointers -- nothing written; n_clips == 0 -> OK.
CPU: the symbol everywhere, the NULL context, and the host half of the plan (tests/cpp/blm_stats_ragged_host.cpp), which pins the
invariant the kernels' waits rest on -- every clip's unit count is a multiple of the kernel's waves.
Every output buffer sits between two guard bands of a NaN-payload sentinel no kernel computes (tests/test_io_dtypes.py: Fence)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_blm_split import TOL, VALID_FRAMES, check_stats, f32, frontend, noise, run_split
from test_io_dtypes import ERR_INVALID_ARG, ERR_UNSUPPORTED, OUT_F32, Fence, _upload

SYMBOL = "melspec_blm_compute_ragged_device_split"
U64P = C.POINTER(C.c_uint64)


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(U64P)


def samples_for(valid, center):
    """a clip length with exactly `valid` valid frames (hop 160, n_fft 512)"""
    if center:
        return (valid - 1) * 160 + (100 if valid == 1 else 0)          # valid = n / 160 + 1
    return 512 + (valid - 1) * 160                                      # valid = (n - 512) / 160 + 1


def flatten(clips):
    """clips back to back with one sample in front of each (odd and even offsets) -> (flat, offsets, lengths)"""
    lens = np.array([len(c) for c in clips], np.uint64)
    offs = (np.concatenate([[0], np.cumsum(lens + 1)[:-1]]) + 1).astype(np.uint64)
    flat = np.full(int(offs[-1] + lens[-1]) + 1, 0.25, np.float32)
    for o, c in zip(offs, clips):
        flat[int(o):int(o) + len(c)] = c
    return flat, offs, lens


def call_ragged(gpu, fe, d_pcm, offs, lens, n_clips, d_rows, rows_offs, d_mean, d_inv_std):
    """the C ABI call; None stays NULL"""
    vp = lambda p: None if p is None else C.c_void_p(p)
    keep = [None if t is None else _u64(t) for t in (offs, lens, rows_offs)]
    tabs = [None if k is None else k[1] for k in keep]
    return gpu._lib.lib().melspec_blm_compute_ragged_device_split(fe._h, vp(d_pcm), tabs[0], tabs[1], n_clips, vp(d_rows), tabs[2], vp(d_mean), vp(d_inv_std), None)


def run_ragged_split(gpu, fe, clips, rows_offs=None, span=None):
    """list of 1-D float32 clips -> ([rows bits [n_mels, cols_c] per clip], mean bits [n_clips, n_mels], inv_std bits [n_clips, n_mels], the
    sentinel): the three outputs fenced; every element of the rows' allocation that belongs to no clip must still be the sentinel, every
    element that does must have been written"""
    nm, n = fe.config.n_mels, len(clips)
    cols = [fe.padded_frames(len(c)) for c in clips]
    sizes = [nm * c for c in cols]
    if rows_offs is None:
        at = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        span = int(sum(sizes))
    else:
        at = np.asarray(rows_offs, np.int64)
    flat, offs, lens = flatten(clips)
    d = _upload(gpu, flat)
    fr, fm, fs = Fence(gpu, max(span, 1), OUT_F32), Fence(gpu, n * nm, OUT_F32), Fence(gpu, n * nm, OUT_F32)
    rc = call_ragged(gpu, fe, d.ptr, offs, lens, n, fr.ptr, rows_offs, fm.ptr, fs.ptr)
    fe.synchronize()
    rows, mean, inv_std = fr.bits(), fm.bits(), fs.bits()          # (checks the guard bands)
    d.free()
    assert rc == 0, gpu._lib.lib().melspec_last_error()
    owned = np.zeros(max(span, 1), bool)
    out = []
    for a, size, c in zip(at, sizes, cols):
        assert not owned[a:a + size].any(), "the test's own offsets overlap"
        owned[a:a + size] = True
        out.append(rows[a:a + size].reshape(nm, c))
    left = (rows == fr.s) & owned
    assert not left.any(), f"rows: {int(left.sum())} elements never written (first at {int(np.argmax(left))})"
    stray = (rows != fr.s) & ~owned
    assert not stray.any(), f"rows: {int(stray.sum())} elements between the clips' rows were written (first at {int(np.argmax(stray))})"
    return out, mean.reshape(n, nm), inv_std.reshape(n, nm), fr.s


def assert_clip_bits(got, want, what):
    for name, a, b in zip(("rows", "mean", "inv_std"), got, want):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        diff = a != b
        assert not diff.any(), f"{what}: {name} differs from the uniform call on the clip alone in {int(diff.sum())} elements (first at {np.argwhere(diff)[0]})"


# ---- the batch of tests 4 and 5, and its yardstick (computed once per configuration, left unchanged) ----------------------------------

_EDGE = {}


def edge_batch(gpu, oracle, nm, mode, center, pad_to):
    """-> (clips, valid frames per clip, [(rows, mean, inv_std) bits of run_split on the clip alone, or None for a frameless clip])"""
    key = (nm, mode, center, pad_to)
    if key not in _EDGE:
        order = np.random.default_rng(4).permutation(len(VALID_FRAMES))
        valid = [VALID_FRAMES[i] for i in order]
        clips = [oracle.synth_pcm(300 + v, samples_for(v, center)) for v in valid]
        # in the middle: a clip without a frame -- center = 0: 300 samples (fewer than n_fft); centred: no sample at all
        valid.insert(6, 0)
        clips.insert(6, oracle.synth_pcm(7, 0 if center else 300))
        fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
        assert fe.supports_split()
        want = []
        for v, x in zip(valid, clips):
            assert fe.num_frames(len(x)) == v
            if v == 0:
                want.append(None)
                continue
            rows, mean, inv_std = run_split(gpu, fe, x[None, :])
            want.append((rows[0].copy(), mean[0].copy(), inv_std[0].copy()))
        fe.close()
        _EDGE[key] = (clips, valid, want)
    return _EDGE[key]


def check_edge_batch(rows, mean, inv_std, sentinel, valid, want, what, stats=True):
    for c, (v, w) in enumerate(zip(valid, want)):
        if v == 0:
            assert rows[c].size == 0
            assert np.all(mean[c] == sentinel) and np.all(inv_std[c] == sentinel), f"{what}: the statistics slots of the frameless clip {c} were written"
            continue
        assert_clip_bits((rows[c], mean[c], inv_std[c]), w, f"{what}, clip {c} ({v} valid frames)")
        assert np.all(rows[c][:, v:] == 0), f"{what}, clip {c}: pad columns are +0"
        if stats:
            check_stats(f32(rows[c]), f32(mean[c]), f32(inv_std[c]), v, f"{what}, clip {c} ({v} valid frames)")


EDGE_PARAMS = dict(argnames="nm,mode,center,pad_to",
                   argvalues=[(nm, mode, center, pad_to) for nm in (80, 128) for mode in ("f64", "f32") for center in (True, False) for pad_to in (0, 16)],
                   ids=lambda v: {True: "center", False: "nocenter"}.get(v, str(v)) if isinstance(v, bool) else str(v))


# ---- Test 4: the bits of the uniform call ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize(**EDGE_PARAMS)
def test_ragged_clips_are_the_uniform_calls_bits(gpu, oracle, nm, mode, center, pad_to):
    clips, valid, want = edge_batch(gpu, oracle, nm, mode, center, pad_to)
    fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
    rows, mean, inv_std, sentinel = run_ragged_split(gpu, fe, clips)
    fe.close()
    check_edge_batch(rows, mean, inv_std, sentinel, valid, want, f"{nm} {mode} pad_to {pad_to} center {center}")


# ---- Test 5: caller offsets -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize(**EDGE_PARAMS)
def test_caller_offsets_reverse_order_with_gaps(gpu, oracle, nm, mode, center, pad_to):
    """the clips' rows in reverse clip order with gaps of 1, 3 and 64 floats in front of them: the same bits, and not one float of the gaps
    (run_ragged_split) or of the guard bands (Fence) touched"""
    clips, valid, want = edge_batch(gpu, oracle, nm, mode, center, pad_to)
    fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97)
    offs, cur = [0] * len(clips), 0
    for k, c in enumerate(reversed(range(len(clips)))):
        cur += (1, 3, 64)[k % 3]
        offs[c] = cur
        cur += nm * fe.padded_frames(len(clips[c]))
    rows, mean, inv_std, sentinel = run_ragged_split(gpu, fe, clips, rows_offs=offs, span=cur + 3)
    fe.close()
    check_edge_batch(rows, mean, inv_std, sentinel, valid, want, f"offsets, {nm} {mode} pad_to {pad_to} center {center}", stats=False)


# ---- Test 6: past one trip of the grid -------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_large_batch_past_one_trip_of_the_grid(gpu, nm, mode):
    """4096 clips of 12 distinct lengths between 0.05 s and 0.6 s (one or two blocks each: at least 4096 rounds for a grid of a workgroup
    per CU) and three clips of 10 s.  Per distinct length one uniform split call on the clips of that length is the yardstick (its own
    position independence: tests/test_blm_split.py); the same ragged batch twice gives the same bits."""
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
        group = noise(n, (len(idx), n))
        rows, mean, inv_std = run_split(gpu, fe, group)
        blocks = -(-fe.padded_frames(n) // (48 if mode == "f32" else 32))
        assert n == 160000 or 1 <= blocks <= 2
        for k, c in enumerate(idx):
            clips[c] = group[k]
            want[c] = (rows[k], mean[k], inv_std[k])
    rows, mean, inv_std, _ = run_ragged_split(gpu, fe, clips)
    for c in range(len(lens)):
        assert_clip_bits((rows[c], mean[c], inv_std[c]), want[c], f"{nm} {mode}: clip {c} of {len(lens)} ({lens[c]} samples)")
    rows2, mean2, inv_std2, _ = run_ragged_split(gpu, fe, clips)
    fe.close()
    assert np.array_equal(mean, mean2) and np.array_equal(inv_std, inv_std2), "the same batch gave other statistics the second time"
    assert all(np.array_equal(a, b) for a, b in zip(rows, rows2)), "the same batch gave other rows the second time"


# ---- Test 7: constant rows ------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_constant_rows_have_no_deviation(gpu, mode):
    fe = frontend(gpu, 128, mode)
    clips = [np.zeros(n, np.float32) for n in (16000, 160, 4800, 7680, 33, 160000, 5120)]
    rows, mean, inv_std, _ = run_ragged_split(gpu, fe, clips)
    fe.close()
    for c, r in enumerate(rows):
        r = f32(r)
        valid = len(clips[c]) // 160 + 1
        assert np.all(r[:, :valid] == r[:, :1]), c
        assert np.array_equal(f32(mean[c]), r[:, 0]) and np.all(f32(inv_std[c]) == np.float32(1e5)), (c, f32(mean[c])[:4], f32(inv_std[c])[:4])


# ---- Test 8: end to end against the oracle --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(), dict(n_mels=128, preemphasis=0.97)])
def test_python_entry_point_matches_the_oracle(gpu, oracle, jfk, kw):
    """blm_compute_ragged_split on the clips of test_blm_split's oracle test, with its numbers (tests/test_gpu_parity.py:
    _check_nemo_normalised): the rows within 1e-4, and on the rows whose f64 std is >= 0.5 the consumer's (rows - mean) * inv_std within
    1e-4 relative to max(1, |z|); every clip has such rows"""
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    cfg_raw = oracle.blm_default_config(**kw)
    cfg_norm = oracle.blm_default_config(normalize_per_feature=1, **kw)
    clips = [jfk, oracle.synth_pcm(2, 16007), oracle.synth_pcm(5, 48000)]
    res = gpu.blm_compute_ragged_split(fe, clips)
    assert len(res) == len(clips)
    for x, (rows, mean, inv_std) in zip(clips, res):
        raw_want, valid = oracle.blm_compute(x, cfg_raw, True)
        want, _ = oracle.blm_compute(x, cfg_norm, True)
        assert rows.shape == want.shape and fe.num_frames(len(x)) == valid
        worst_raw = float(np.abs(rows - raw_want).max())
        got = np.zeros_like(rows)
        got[:, :valid] = (rows[:, :valid] - mean[:, None]) * inv_std[:, None]
        std = raw_want[:, :valid].astype(np.float64).std(axis=1, ddof=1)
        good = std >= 0.5
        gated = int(good.sum())
        d = np.abs(got[good] - want[good]) / np.maximum(1.0, np.abs(want[good]))
        print(f"{kw} {len(x)} samples: rows worst {worst_raw:.3e}; {gated} rows gated, worst {float(d.max()) if gated else float('nan'):.3e}")
        assert worst_raw <= TOL, worst_raw
        assert gated > 0
        assert d.max() <= TOL, float(d.max())
    empty = gpu.blm_compute_ragged_split(fe, [clips[1], np.zeros(0, np.float32)])
    assert empty[1][0].shape == (fe.config.n_mels, 0) and empty[1][1] is None and empty[1][2] is None
    assert np.array_equal(empty[0][0], res[1][0]) and np.array_equal(empty[0][1], res[1][1]) and np.array_equal(empty[0][2], res[1][2])
    fe.close()


# ---- Test 9: refusals -----------------------------------------------------------------------------------------------------------------

def _refused(gpu, fe, clips, null=(), n_clips=None):
    """the call with the arguments named in `null` passed as NULL -> its status; none of the three fenced outputs may have been written"""
    nm, n = fe.config.n_mels, len(clips)
    flat, offs, lens = flatten(clips)
    d = _upload(gpu, flat)
    fr = Fence(gpu, max(sum(nm * fe.padded_frames(len(c)) for c in clips), 1), OUT_F32)
    fm, fs = Fence(gpu, n * nm, OUT_F32), Fence(gpu, n * nm, OUT_F32)
    arg = dict(pcm=d.ptr, offs=offs, lens=lens, rows=fr.ptr, mean=fm.ptr, inv_std=fs.ptr)
    for k in null:
        arg[k] = None
    rc = call_ragged(gpu, fe, arg["pcm"], arg["offs"], arg["lens"], n if n_clips is None else n_clips, arg["rows"], None, arg["mean"], arg["inv_std"])
    fe.synchronize()
    for name, f in (("rows", fr), ("mean", fm), ("inv_std", fs)):
        b = f.bits()
        assert np.all(b == f.s), f"{name}: a call that computes nothing wrote {int((b != f.s).sum())} elements"
    d.free()
    return rc


@pytest.mark.gpu
def test_refusals_write_nothing(gpu, oracle):
    last = lambda: gpu._lib.lib().melspec_last_error().decode()
    clips = [oracle.synth_pcm(c, n) for c, n in enumerate((4000, 1234))]
    for kw in (dict(n_mels=40), dict(n_mels=80, n_fft=1024, win_length=800, hop_length=256), dict(n_mels=80, n_fft=512, win_length=320)):
        fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
        assert not fe.supports_split(), kw
        assert _refused(gpu, fe, clips) == ERR_UNSUPPORTED
        msg = last()
        assert "split output" in msg and f"n_mels = {kw['n_mels']}" in msg and f"n_fft = {kw.get('n_fft', 512)}" in msg, msg
        # unsupported comes before everything but the NULL context: also without clips, tables or pointers
        assert _refused(gpu, fe, clips, null=("offs", "lens", "pcm", "rows", "mean", "inv_std"), n_clips=0) == ERR_UNSUPPORTED
        with pytest.raises(Exception):
            gpu.blm_compute_ragged_split(fe, clips)
        fe.close()
    for nm, mode in ((80, "f64"), (128, "f32")):
        fe = frontend(gpu, nm, mode, center=False)
        assert fe.supports_split()
        assert _refused(gpu, fe, clips, null=("offs", "lens", "pcm", "rows", "mean", "inv_std"), n_clips=0) == 0          # no clips: OK
        for tab in ("offs", "lens"):
            assert _refused(gpu, fe, clips, null=(tab,)) == ERR_INVALID_ARG
            assert "offset/length" in last()
        for ptr in ("pcm", "rows", "mean", "inv_std"):
            assert _refused(gpu, fe, clips, null=(ptr,)) == ERR_INVALID_ARG, ptr
            assert "NULL" in last()
        # no valid frame in the whole batch (center = 0, fewer than n_fft samples): OK, nothing written, the pointers are not looked at
        short = [oracle.synth_pcm(c, n) for c, n in enumerate((300, 0, 511))]
        assert _refused(gpu, fe, short) == 0
        assert _refused(gpu, fe, short, null=("pcm", "rows", "mean", "inv_std")) == 0
        assert _refused(gpu, fe, short, null=("offs",)) == ERR_INVALID_ARG              # ... but the tables are
        fe.close()


# ---- CPU ------------------------------------------------------------------------------------------------------------------------------

def test_ragged_split_symbol_everywhere():
    """the entry point resolves in the built library and is declared in the header, the ctypes table, the C++ wrapper and the Rust shim;
    the ABI version is still 1 and the header is still C99"""
    from mel_spec_amd import _lib
    import mel_spec_amd
    lib = _lib.lib()
    header_path = os.path.join(ROOT, "include", "melspec_hip.h")
    header = open(header_path).read()
    table = open(os.path.join(ROOT, "mel_spec_amd", "_lib.py")).read()
    wrapper = open(os.path.join(ROOT, "include", "melspec_hip.hpp")).read()
    shim = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    assert getattr(lib, SYMBOL) is not None
    assert SYMBOL in _lib.SIGNATURES
    assert re.search(rf"\b{SYMBOL}\s*\(", header)
    assert f'"{SYMBOL}"' in table
    assert re.search(rf"\b{SYMBOL}\s*\(", wrapper)
    assert re.search(rf"\bfn {SYMBOL}\s*\(", shim) and re.search(r"\bunsafe fn compute_ragged_device_split\s*\(", shim)
    assert "no ragged form" not in header
    assert callable(mel_spec_amd.blm_compute_ragged_device_split) and callable(mel_spec_amd.blm_compute_ragged_split)
    assert lib.melspec_abi_version() == 1
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-x", "c", header_path])


def test_ragged_split_null_context_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    tab, tp = _u64([0])
    ln, lp = _u64([1024])
    assert lib.melspec_blm_compute_ragged_device_split(None, p, tp, lp, 1, p, None, p, p, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_compute_ragged_device_split(None, None, None, None, 0, None, None, None, None, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert np.all(buf == 0)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_ragged_split_plan_and_arguments_on_the_host(tmp_path, sanitize):
    """the arithmetic half of the host side (mel_spec_amd/csrc/blm_stats_plan.hpp: blm_stats_plan_ragged, the units plan_ragged gives a clip,
    the argument verdicts) as a stand-alone program, plain and with -fsanitize=address,undefined: tests/cpp/blm_stats_ragged_host.cpp"""
    exe = tmp_path / "blm_stats_ragged_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blm_stats_ragged_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("blm_stats_ragged_host: ok"), p.stdout + p.stderr
