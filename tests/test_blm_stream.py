"""The NeMo / Parakeet frontend's stream bank (melspec_blm_stream_*): BatchLogMelSpectrogram::compute (src/mel.rs) fed chunk by chunk with
the sample history on the device -- un-normalised feature-major columns, bit-identical to the batch call on the concatenated samples
however they were cut, the zero-padded last columns at finish, plus the running per-feature mean and 1 / (std + 1e-5).  The CPU part
drives the bookkeeping (csrc/blm_stream_plan.hpp) with the kernel's rule for a tap standing in for the kernel
(tests/cpp/blm_stream_host.cpp) and the argument checks that need no device; the GPU part drives the real thing.

Tolerances.  Between the bank and the library's own batch call, and between two cuts of the same samples: bit equality.  Against
oracle.blm_compute: what the existing NeMo parity tests use for the mode -- TOL = 1e-4 in the default f64 mode (tests/test_gpu_parity.py),
tests/test_f32_512.py's _nemo_gate (the distance of the reference's own f32 arithmetic from the f64 evaluation) in MELSPEC_PRECISION_F32.
stats against the numpy restatement of the f64 Welford fold over the bank's own columns: 1 ulp of f32 (the fold is IEEE f64 on both
sides; the ulp is for the final square root, reciprocal and rounding).  (rows - mean) * inv_std against the split call's: that call's
statistics are gated at 1e-5 of max|row| for the mean and 1e-5 relative for inv_std against f64 statistics (tests/test_blm_split.py,
check_stats), so are the bank's here, and on the rows that test gates end to end (f64 std >= 0.5) the two normalisations agree within
its 1e-4 relative to max(1, |z|)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT

TOL = 1e-4

SYMBOLS = ["melspec_blm_stream_create", "melspec_blm_stream_destroy", "melspec_blm_stream_reset", "melspec_blm_stream_frames_after",
           "melspec_blm_stream_finish_frames", "melspec_blm_stream_input_ptr", "melspec_blm_stream_push_host", "melspec_blm_stream_push_device",
           "melspec_blm_stream_finish_host", "melspec_blm_stream_finish_device", "melspec_blm_stream_stats_host", "melspec_blm_stream_stats_device"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def host_run(request, tmp_path_factory):
    """tests/cpp/blm_stream_host.cpp, built with the host compiler -- plain and with -fsanitize=address,undefined (a stand-alone
    program) -- and run once each"""
    exe = tmp_path_factory.mktemp("blm_stream") / "blm_stream_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blm_stream_host.cpp"), "-o", str(exe)])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)


def test_bank_bookkeeping_on_the_host(host_run):
    """hops 160, 120, 400, 1 x center 0, 1 x max_chunk 160, 517, 2000; chunk sizes from {0, 1, hop - 1, hop, hop + 1, 199, 200, 201, 399,
    400, 401, max_chunk} to a random subset of 5 streams per push, then a finish: every emitted frame's 400 taps read through (off, len,
    org0_i) with the kernel's rule are the taps of the whole clip (zero outside [0, len), no predecessor at the stream's sample 0 only),
    frame counts are frames_after / finish_frames and sum to num_frames(total), the carry stays below 401 / 457 <= in_off, an ended
    stream refuses a push, a refused call changes nothing."""
    assert host_run.returncode == 0 and "blm_stream_host: ok" in host_run.stdout, host_run.stdout[-4000:] + host_run.stderr[-2000:]


def test_first_pushes_of_one_hop(host_run):
    """centred, hop 160: frame k is there with k * 160 + 200 samples; the finish after 800 samples emits frames 4 and 5"""
    m = re.search(r"^first_pushes(( \d+)+) finish (\d+)$", host_run.stdout, flags=re.M)
    assert m, host_run.stdout[-2000:]
    assert [int(v) for v in m.group(1).split()] == [0, 1, 1, 1, 1] and int(m.group(3)) == 2


def test_errors_without_a_device():
    """NULL handles and zero sizes are refused before any device is touched; id out of range / an id twice / an over-long chunk / an ended
    stream are the plan header's refusals (checked in test_bank_bookkeeping_on_the_host: codes 1, 1, 2, 1)"""
    from mel_spec_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    u32 = (C.c_uint32 * 2)(0, 1)
    f32 = (C.c_float * 8)()
    u64 = (C.c_uint64 * 2)()
    assert L.melspec_blm_stream_create(None, None, 4, 160) == _lib.ERR_INVALID_ARG and "out is NULL" in _lib.last_error()
    assert L.melspec_blm_stream_create(C.byref(h), None, 0, 160) == _lib.ERR_INVALID_ARG and "must be > 0" in _lib.last_error()
    assert L.melspec_blm_stream_create(C.byref(h), None, 4, 0) == _lib.ERR_INVALID_ARG and "must be > 0" in _lib.last_error()
    assert L.melspec_blm_stream_create(C.byref(h), None, 4, 160) == _lib.ERR_INVALID_ARG and "blm is NULL" in _lib.last_error()
    assert not h.value
    calls = [
        lambda: L.melspec_blm_stream_reset(None, None, 0),
        lambda: L.melspec_blm_stream_push_host(None, u32, f32, 0, u32, 1, f32, 8, u32),
        lambda: L.melspec_blm_stream_push_device(None, u32, None, 0, None, u32, 1, None, None, u32, None),
        lambda: L.melspec_blm_stream_finish_host(None, u32, 1, f32, 8, u32),
        lambda: L.melspec_blm_stream_finish_device(None, u32, 1, None, None, u32, None),
        lambda: L.melspec_blm_stream_stats_host(None, u32, 1, f32, f32, u64),
        lambda: L.melspec_blm_stream_stats_device(None, u32, 1, None, None, u64, None),
    ]
    # the handle is looked at first: before n == 0, before NULL ids / lens / samples / mean / inv_std, before the dtype codes
    assert L.melspec_blm_stream_create(None, None, 0, 0) == _lib.ERR_INVALID_ARG and "out is NULL" in _lib.last_error()
    calls += [
        lambda: L.melspec_blm_stream_push_host(None, None, None, 0, None, 0, None, 0, None),
        lambda: L.melspec_blm_stream_push_host(None, None, None, 7, None, 1, None, 0, None),
        lambda: L.melspec_blm_stream_push_device(None, None, None, 1, None, None, 1, None, None, None, None),
        lambda: L.melspec_blm_stream_finish_host(None, None, 0, None, 0, None),
        lambda: L.melspec_blm_stream_finish_host(None, None, 1, None, 0, None),
        lambda: L.melspec_blm_stream_finish_device(None, None, 1, None, None, None, None),
        lambda: L.melspec_blm_stream_stats_host(None, None, 0, None, None, None),
        lambda: L.melspec_blm_stream_stats_host(None, None, 1, None, None, None),
        lambda: L.melspec_blm_stream_stats_device(None, None, 1, None, None, None, None),
    ]
    # a handle of another bank (the Kaldi bank's tag in its first word) reads as NULL
    other = (C.c_uint32 * 16)(0x4B53424D)
    calls += [
        lambda: L.melspec_blm_stream_reset(other, None, 0),
        lambda: L.melspec_blm_stream_push_host(other, u32, f32, 0, u32, 1, f32, 8, u32),
        lambda: L.melspec_blm_stream_finish_host(other, u32, 1, f32, 8, u32),
        lambda: L.melspec_blm_stream_stats_host(other, u32, 1, f32, f32, u64),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID_ARG, k
        assert "blm stream bank is NULL" in _lib.last_error(), (k, _lib.last_error())
    for h_bad in (None, other):
        assert L.melspec_blm_stream_frames_after(h_bad, 0, 400) == 0 and L.melspec_blm_stream_finish_frames(h_bad, 0) == 0
        assert not L.melspec_blm_stream_input_ptr(h_bad, 0)
        assert L.melspec_blm_stream_supports_io(h_bad, 0, 0) == 0
        L.melspec_blm_stream_destroy(h_bad)
    assert other[0] == 0x4B53424D and not any(other[i] for i in range(1, 16))


def test_symbols_are_exported_and_bound():
    from mel_spec_amd import _lib
    L = _lib.lib()
    rs = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "melspec_hip.hpp")).read()
    hdr = open(os.path.join(ROOT, "include", "melspec_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
        assert re.search(r"\b%s\s*\(" % s, hdr), s
        assert re.search(r"fn\s+%s\s*\(" % s, rs), f"{s} is not bound in hip.rs"
        assert re.search(r"\b%s\s*\(" % s, hpp), f"{s} is not used by melspec_hip.hpp"
    import mel_spec_amd as M
    assert hasattr(M, "BlmStreamBank")
    for m in ("push", "finish", "push_device", "finish_device", "stats", "stats_device"):
        assert callable(getattr(M.BlmStreamBank, m))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _sources(jfk, n_streams=7, n=24000):
    return [np.ascontiguousarray(jfk[(7919 * s) % 60000:][:n] * np.float32(1.0 + 0.1 * s)) for s in range(n_streams)]


def _frontend(gpu, mode, **kw):
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    fe.set_precision(mode)
    return fe


def _drive(bank, src, hop, max_chunk, seed):
    """tests/test_fbank_stream.py's _drive for this bank: random-sized chunks (incl. sizes below, at and above a hop, half a window and a
    window) to a random subset of the streams per push, then one finish of all streams in two calls; returns every stream's
    concatenated columns [n_mels, k]"""
    rng = np.random.default_rng(seed)
    n_streams = len(src)
    pos = [0] * n_streams
    got = [[np.zeros((bank.n_mels, 0), np.float32)] for _ in range(n_streams)]
    sizes = [0, 1, hop - 1, hop, hop + 1, 2 * hop, 199, 200, 201, 399, 400, 401, max_chunk]
    live = set(range(n_streams))
    while live:
        ids = [s for s in sorted(live) if rng.random() < 0.7]
        if not ids:
            continue
        chunks = []
        for s in ids:
            n = int(rng.choice(sizes)) if rng.random() < 0.5 else int(rng.integers(0, max_chunk + 1))
            n = min(n, max_chunk, len(src[s]) - pos[s])
            chunks.append(src[s][pos[s]:pos[s] + n]); pos[s] += n
        want_counts = [bank.frames_after(s, len(c)) for s, c in zip(ids, chunks)]
        res = bank.push(ids, chunks)
        assert [r.shape for r in res] == [(bank.n_mels, k) for k in want_counts]
        for s, r in zip(ids, res):
            got[s].append(r.copy())
            if pos[s] >= len(src[s]):
                live.discard(s)
    order = [int(s) for s in rng.permutation(n_streams)]
    for ids in (order[:3], order[3:]):
        want_counts = [bank.finish_frames(s) for s in ids]
        res = bank.finish(ids)
        assert [r.shape for r in res] == [(bank.n_mels, k) for k in want_counts]
        for s, r in zip(ids, res):
            got[s].append(r.copy())
    return [np.concatenate(g, axis=1) for g in got]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _welford(cols):
    """the numpy restatement of the bank's statistics: Welford's update in f64, one column at a time in time order ->
    (mean f32, inv_std f32) per row of [n_mels, k]"""
    nm, k = cols.shape
    mean, m2 = np.zeros(nm, np.float64), np.zeros(nm, np.float64)
    for f in range(k):
        x = cols[:, f].astype(np.float64)
        d = x - mean
        mean = mean + d / np.float64(f + 1)
        m2 = m2 + d * (x - mean)
    inv = 1.0 / (np.sqrt(m2 / np.float64(max(k - 1, 1))) + 1e-5)
    return mean.astype(np.float32), inv.astype(np.float32)


def _within_one_ulp(got, want):
    return bool(np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)))


CONFIGS = [
    ("80_f64", dict(), "f64", 1000, False),
    ("128_f64_preemph", dict(n_mels=128, preemphasis=0.97), "f64", 1000, False),
    ("80_f32_preemph", dict(preemphasis=0.97), "f32", 1000, False),
    ("128_f32", dict(n_mels=128), "f32", 517, False),
    ("nocenter_f64_preemph", dict(center=False, preemphasis=0.97), "f64", 1000, False),
    ("nocenter_128_f32", dict(center=False, n_mels=128), "f32", 700, False),
    ("runtime_bank", dict(f_min=100.0, preemphasis=0.97), "f64", 700, False),
    ("int16", dict(preemphasis=0.97), "f64", 640, True),
    ("int16_f32", dict(n_mels=128, preemphasis=0.97), "f32", 640, True),
    ("hop_120", dict(hop_length=120, preemphasis=0.97), "f64", 517, False),
    ("hop_120_f32", dict(hop_length=120), "f32", 517, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,mode,max_chunk,s16", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_random_chunks_rows_and_stats(gpu, oracle, jfk, name, kw, mode, max_chunk, s16):
    """7 streams of 24 000 JFK samples, each scaled differently, two seeds (two different cuts of the same sources), then finish: columns
    bit-equal to the batch call of a normalize_per_feature = 0 twin on the concatenation and between the cuts, within the mode's
    tolerance of the oracle; stats bit-equal between the cuts and between stats_host and stats_device, within 1 ulp of the numpy Welford
    fold over the bank's own columns; and against the split call as the module's header says.  The bank stands on a context with
    normalize_per_feature = 1 and pad_to = 16: neither matters to it."""
    from test_f32_512 import _nemo_gate
    src = _sources(jfk)
    if s16:
        q = [np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) for x in src]
        src, as_f32 = q, [x.astype(np.float32) * np.float32(2.0 ** -15) for x in q]
    else:
        as_f32 = src
    fe = _frontend(gpu, mode, normalize_per_feature=True, pad_to=16, **kw)
    twin = _frontend(gpu, mode, normalize_per_feature=False, **kw)
    want_mode = mode if name != "runtime_bank" else "f64"
    assert fe.precision == want_mode and twin.precision == want_mode
    hop, nm = fe.config.hop_length, fe.config.n_mels
    ocfg = oracle.blm_default_config(**{k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()})
    ids = list(range(len(src)))
    runs = []
    for seed in (11, 12):
        bank = gpu.BlmStreamBank(fe, len(src), max_chunk)
        cols = _drive(bank, src, hop, max_chunk, seed)
        mean, inv_std, counts = bank.stats(ids)
        d_mean, d_inv = gpu.DeviceBuffer(mean.nbytes), gpu.DeviceBuffer(mean.nbytes)
        counts_d = bank.stats_device(ids, d_mean.ptr, d_inv.ptr)
        mean_d, inv_d = d_mean.download(mean.shape), d_inv.download(mean.shape)
        d_mean.free(); d_inv.free(); bank.close()
        assert np.array_equal(counts, counts_d) and np.array_equal(_bits(mean), _bits(mean_d)) and np.array_equal(_bits(inv_std), _bits(inv_d))
        runs.append((cols, mean, inv_std, counts))
    worst = worst_z = worst_dm = worst_ds = 0.0
    for s in ids:
        (c1, m1, i1, n1), (c2, m2, i2, _) = runs
        batch = twin.compute(as_f32[s])
        want, valid = oracle.blm_compute(as_f32[s], ocfg, True)
        assert c1[s].shape == batch.shape == want.shape == (nm, valid) and int(n1[s]) == valid
        assert np.array_equal(_bits(c1[s]), _bits(batch)), (name, s, "columns differ from the batch call", int((_bits(c1[s]) != _bits(batch)).sum()))
        assert np.array_equal(_bits(c1[s]), _bits(c2[s])), (name, s, "another cut, other columns")
        assert np.array_equal(_bits(m1[s]), _bits(m2[s])) and np.array_equal(_bits(i1[s]), _bits(i2[s])), (name, s, "another cut, other statistics")
        wm, wi = _welford(c1[s])
        assert _within_one_ulp(m1[s], wm) and _within_one_ulp(i1[s], wi), (name, s, "statistics are not the Welford fold of the columns")
        if want_mode == "f32":
            lit, _ = oracle.blm_compute(as_f32[s], ocfg, False)
            d, gate = _nemo_gate(c1[s], want, lit)
        else:
            d, gate = float(np.abs(c1[s] - want).max()), TOL
        worst = max(worst, d / gate)
        # the statistics against f64 statistics of the columns, with the split call's margins ...
        x64 = c1[s].astype(np.float64)
        mean64 = x64.mean(axis=1)
        inv64 = 1.0 / (np.sqrt(((x64 - mean64[:, None]) ** 2).sum(axis=1) / max(valid - 1, 1)) + 1e-5)
        worst_dm = max(worst_dm, float((np.abs(m1[s] - mean64) / np.abs(c1[s]).max(axis=1)).max()) / 1e-5)
        worst_ds = max(worst_ds, float((np.abs(i1[s] - inv64) / inv64).max()) / 1e-5)
        # ... and the normalisation against the split call's own, where it exists
        if twin.supports_split():
            rows_s, mean_s, inv_s = twin.compute_split(as_f32[s])
            assert np.array_equal(_bits(rows_s[:, :valid]), _bits(c1[s]))
            good = x64.std(axis=1, ddof=1) >= 0.5
            assert good.any()
            z = (c1[s] - m1[s][:, None]) * i1[s][:, None]
            z_s = (rows_s[:, :valid] - mean_s[:, None]) * inv_s[:, None]
            worst_z = max(worst_z, float((np.abs(z[good] - z_s[good]) / np.maximum(1.0, np.abs(z_s[good]))).max()) / TOL)
    print(f"{name}: rows {worst:.3f} mean {worst_dm:.3f} inv_std {worst_ds:.3f} normalised vs split {worst_z:.3f} (fractions of their bounds)")
    assert worst <= 1.0 and worst_dm <= 1.0 and worst_ds <= 1.0 and worst_z <= 1.0
    fe.close(); twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_gpu_stream_ends(gpu, oracle, jfk, mode):
    """streams of 1, 159, 160, 199, 200, 201 and 360 samples pushed in one go and finished: 1, 1, 2, 2, 2, 2 and 3 columns, the bits of the
    batch call; an empty stream finished emits nothing; a second finish and a push after finish are INVALID_ARG and leave the bank as
    it was (the statistics stay readable); reset starts the stream afresh"""
    from mel_spec_amd import _lib
    lens = [1, 159, 160, 199, 200, 201, 360]
    fe = _frontend(gpu, mode, preemphasis=0.97)
    assert fe.precision == mode
    src = [np.ascontiguousarray(jfk[30000 + 1000 * i:][:n]) for i, n in enumerate(lens)]
    bank = gpu.BlmStreamBank(fe, len(lens) + 1, 400)
    ids = list(range(len(lens)))
    empty = len(lens)
    pushed = bank.push(ids, src)
    assert [r.shape[1] for r in pushed] == [0, 0, 0, 0, 1, 1, 2]
    assert [bank.finish_frames(s) for s in ids + [empty]] == [1, 1, 2, 2, 1, 1, 1, 0]
    finished = bank.finish(ids + [empty])
    assert finished[empty].shape == (80, 0)
    for s, n in enumerate(lens):
        got = np.concatenate([pushed[s], finished[s]], axis=1)
        want = fe.compute(src[s])
        assert got.shape == want.shape == (80, [1, 1, 2, 2, 2, 2, 3][s]), (n, got.shape, want.shape)
        assert np.array_equal(_bits(got), _bits(want)), (n, "columns differ from the batch call")
    mean, inv_std, counts = bank.stats(ids + [empty])
    assert list(counts) == [1, 1, 2, 2, 2, 2, 3, 0]
    assert np.all(mean[empty] == 0) and np.all(inv_std[empty] == np.float32(1e5))
    assert np.array_equal(_bits(mean[0]), _bits(fe.compute(src[0])[:, 0])) and np.all(inv_std[0] == np.float32(1e5))      # one column: var = 0
    for s in (0, 6, empty):
        assert bank.frames_after(s, 400) == 0 and bank.finish_frames(s) == 0
        with pytest.raises(gpu.HipError) as e:
            bank.finish([s])
        assert e.value.code == _lib.ERR_INVALID_ARG and "finished" in str(e.value)
        with pytest.raises(gpu.HipError) as e:
            bank.push([s], [src[3]])
        assert e.value.code == _lib.ERR_INVALID_ARG and "finished" in str(e.value)
    again = bank.stats(ids + [empty])
    assert all(np.array_equal(a, b) for a, b in zip(again, (mean, inv_std, counts)))
    bank.reset([6, empty])
    a, b = bank.push([6, empty], [src[6], src[4]])
    assert np.array_equal(_bits(a), _bits(pushed[6])) and np.array_equal(_bits(b), _bits(pushed[4]))
    assert list(bank.stats([6, empty])[2]) == [2, 1]
    bank.close(); fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
def test_gpu_chunk_borders_nonfinite(gpu, oracle, jfk, poison, center):
    """pre-emphasis across chunk borders: a NaN or an infinity at the stream's sample 0, at the last sample of a chunk, at the first of the
    next and at the predecessor of a frame's first tap reaches exactly the columns it reaches in the batch call -- bit for bit, in two
    different cuts"""
    fe = _frontend(gpu, "f64", preemphasis=0.97, center=center)
    clean = np.ascontiguousarray(jfk[20000:21000])
    first_tap = 3 * 160 + (-200 if center else 56)                    # frame 3's
    spots = [0, first_tap - 1, first_tap, 359, 360, 519, 520]
    src = []
    for p in spots:
        x = clean.copy(); x[p] = poison
        src.append(x)
    ids = list(range(len(spots)))
    want = [fe.compute(x) for x in src]
    for cuts in ((360, 160, 480), (first_tap, 1, 300, 1000 - first_tap - 301)):
        bank = gpu.BlmStreamBank(fe, len(spots), 600)
        got = [[] for _ in ids]
        lo = 0
        for n in cuts:
            for s, r in zip(ids, bank.push(ids, [x[lo:lo + n] for x in src])):
                got[s].append(r)
            lo += n
        assert lo == 1000
        for s, r in zip(ids, bank.finish(ids)):
            got[s].append(r)
        for s in ids:
            mine = np.concatenate(got[s], axis=1)
            assert mine.shape == want[s].shape
            assert not np.isfinite(want[s]).all() or center is False and spots[s] < 56, (spots[s], "the poison reached no column of the batch call")
            assert np.array_equal(_bits(mine), _bits(want[s])), (cuts, spots[s], np.argwhere(_bits(mine) != _bits(want[s]))[:4])
        bank.close()
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_gpu_past_one_grid_trip_device_pushes(gpu, oracle, jfk, mode):
    """more entries in one device push than the resident workgroups hold in one trip (CUs x 8 f64 waves, CUs x 12 f32 waves; one unit per
    entry): every stream is fed one of 5 scaled sources as 200 + 160 + 160 samples from a device buffer and finished, each call emitting
    one column per stream at caller-placed offsets into a fenced buffer: every column of every stream is bit-equal to its source's
    batch column and nothing outside the columns is written."""
    nm = 80
    waves = 12 if mode == "f32" else 8
    n_streams = torch.cuda.get_device_properties(0).multi_processor_count * waves + 137
    fe = _frontend(gpu, mode, preemphasis=0.97)
    assert fe.precision == mode
    srcs = [np.ascontiguousarray(jfk[(7919 * s) % 60000:][:520] * np.float32(1.0 + 0.1 * s)) for s in range(5)]
    want = [fe.compute(x) for x in srcs]                  # 520 samples: 4 columns
    assert all(w.shape == (nm, 4) for w in want)
    bank = gpu.BlmStreamBank(fe, n_streams, 200)
    ids = np.arange(n_streams, dtype=np.uint32)
    # the column of stream s at (s * 3 + 1) * nm floats: a column of fence in front of the first stream's, two behind every stream's
    FENCE = np.float32(-777.0)
    out = gpu.DeviceBuffer((n_streams * 3 + 1) * nm * 4)
    offs = (np.arange(n_streams, dtype=np.uint64) * 3 + 1) * nm
    d_chunks = gpu.DeviceBuffer(n_streams * 200 * 4)
    pos = 0
    for col, n in enumerate((200, 160, 160, 0)):
        out.upload(np.full((n_streams * 3 + 1) * nm, FENCE, np.float32))
        if n:
            d_chunks.upload(np.ascontiguousarray(np.stack([srcs[s % 5][pos:pos + n] for s in range(n_streams)])))
            fr = bank.push_device(ids, np.full(n_streams, n, np.uint32), out.ptr, out_offsets=offs, d_chunks=d_chunks.ptr)
        else:
            fr = bank.finish_device(ids, out.ptr, out_offsets=offs)
        assert (fr == 1).all()
        got = out.download((n_streams * 3 + 1, nm))
        mine = got[1:].reshape(n_streams, 3, nm)
        for s in range(5):
            assert np.array_equal(_bits(mine[s::5, 0]), np.broadcast_to(_bits(want[s][:, col]), mine[s::5, 0].shape)), (col, s)
        assert (mine[:, 1:] == FENCE).all() and (got[0] == FENCE).all(), col
        pos += n
    mean, inv_std, counts = bank.stats(ids)
    assert (counts == 4).all()
    for s in range(5):
        wm, wi = _welford(want[s])
        assert (_bits(mean[s::5]) == _bits(mean[s])).all() and (_bits(inv_std[s::5]) == _bits(inv_std[s])).all()
        assert _within_one_ulp(mean[s], wm) and _within_one_ulp(inv_std[s], wi)
    out.free(); d_chunks.free(); bank.close(); fe.close()


@pytest.mark.gpu
def test_gpu_unsupported_geometry_and_refused_pushes(gpu, oracle, jfk):
    """a context off the fused path is refused at create with the geometry in the message; refused pushes (id out of range, an id twice, an
    over-long chunk) change nothing"""
    from mel_spec_amd import _lib
    L = _lib.lib()
    slow = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(win_length=320))
    h = C.c_void_p()
    assert L.melspec_blm_stream_create(C.byref(h), slow._h, 4, 160) == _lib.ERR_UNSUPPORTED and not h.value
    assert "win_length = 320" in _lib.last_error() and "n_fft = 512" in _lib.last_error()
    slow.close()
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig())
    bank = gpu.BlmStreamBank(fe, 2, 600)
    x = np.ascontiguousarray(jfk[7000:7800])
    a = bank.push([0], [x[:300]])[0]
    for ids, chunks, code in (([2], [x[:10]], _lib.ERR_INVALID_ARG), ([0, 0], [x[:10], x[:10]], _lib.ERR_INVALID_ARG),
                              ([1, 0], [x[:10], x[:601]], _lib.ERR_CAPACITY)):
        with pytest.raises(gpu.HipError) as e:
            bank.push(ids, chunks)
        assert e.value.code == code, (ids, str(e.value))
    b = bank.push([0], [x[300:800]])[0]
    c = bank.finish([0])[0]
    assert np.array_equal(_bits(np.concatenate([a, b, c], axis=1)), _bits(fe.compute(x)))
    assert bank.stats([1])[2][0] == 0 and bank.frames_after(1, 200) == 1           # stream 1, named in a refused push, never received a sample
    bank.close(); fe.close()


@pytest.mark.gpu
def test_gpu_reset_with_a_bad_id_resets_nothing(gpu, oracle, jfk):
    """melspec_blm_stream_reset checks every id before it touches anything: reset([0, 7]) on a bank of two streams is INVALID_ARG and
    stream 0, listed in front of the bad id, goes on where it was -- both streams' columns are the batch call's, bit for bit, and so are
    the statistics of a bank that was never disturbed."""
    from mel_spec_amd import _lib
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(preemphasis=0.97))
    src = [np.ascontiguousarray(jfk[20000:20000 + 960]), np.ascontiguousarray(jfk[41000:41000 + 960])]
    runs = []
    for disturb in (True, False):
        bank = gpu.BlmStreamBank(fe, 2, 400)
        got = [[], []]
        for k in range(6):
            if k == 3 and disturb:
                with pytest.raises(gpu.HipError) as e:
                    bank.reset([0, 7])
                assert e.value.code == _lib.ERR_INVALID_ARG and "out of range" in str(e.value)
            for i, r in enumerate(bank.push([0, 1], [s[k * 160:(k + 1) * 160] for s in src])):
                got[i].append(r)
        for i, r in enumerate(bank.finish([0, 1])):
            got[i].append(r)
        runs.append(([np.concatenate(g, axis=1) for g in got], bank.stats([0, 1])))
        bank.close()
    for i in range(2):
        want = fe.compute(src[i])
        assert want.shape == (80, 7) and np.array_equal(_bits(runs[0][0][i]), _bits(want)), i
    assert all(np.array_equal(a, b) for a, b in zip(runs[0][1], runs[1][1]))
    fe.close()
