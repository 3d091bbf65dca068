"""The Kaldi fbank's stream bank (melspec_fbank_stream_*): Fbank::compute (src/fbank.rs:141-236) fed chunk by chunk with the frame
history on the device -- rows before CMN, bit-identical to the batch call on the concatenated samples however they were cut, plus the
running column means.  The CPU part drives the bookkeeping (csrc/fbank_stream_plan.hpp) with the oracle standing in for the kernel
(tests/cpp/fbank_stream_host.cpp) and the argument checks that need no device; the GPU part drives the real thing.

Tolerances.  TOL = 1e-4 against the oracle is the fused fbank path's existing gate (tests/test_gpu_parity.py): absolute on log
energies, and 1e-4 * max(1, |want|.max()) where use_log_fbank is off (linear energies of a few hundred have an f32 ulp of 6e-5; the
same expression as test_fbank_variants_and_edges).  Everything between the bank and the library's own batch call is bit equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

TOL = 1e-4
FLOOR_ROW = np.float32(np.log(np.float32(np.finfo(np.float32).eps)))        # ln(f32::EPSILON) = -15.942385

SYMBOLS = ["melspec_fbank_stream_create", "melspec_fbank_stream_destroy", "melspec_fbank_stream_reset", "melspec_fbank_stream_frames_after",
           "melspec_fbank_stream_push_host", "melspec_fbank_stream_input_ptr", "melspec_fbank_stream_push_device",
           "melspec_fbank_stream_stats_host", "melspec_fbank_stream_stats_device"]


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan_ubsan"])
def host_run(request, oracle, tmp_path_factory):
    """tests/cpp/fbank_stream_host.cpp, built with the host compiler against the oracle's library -- plain and with
    -fsanitize=address,undefined (a stand-alone program) -- and run once each"""
    odir = os.path.join(ROOT, "oracle")
    exe = tmp_path_factory.mktemp("fbank_stream") / "fbank_stream_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if request.param else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "fbank_stream_host.cpp"), "-o", str(exe), "-L", odir, "-l:libmelspec_oracle.so",
                           "-Wl,-rpath," + odir])
    return subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)


def test_bank_bookkeeping_on_the_host(host_run):
    """shifts 160, 120, 400, 1 x max_chunk 160, 517, 2000; chunk sizes from {0, 1, shift - 1, shift, shift + 1, 239, 240, 241, 399, 400,
    401, max_chunk} to a random subset of 5 streams per push: every stream's concatenated rows are oracle.fbank_compute(x, apply_cmn = 0)
    in shape and bits, frames_after agrees with every push, the continues flag of every entry is "the stream has emitted", keep <=
    frame_len, and the carry holds the predecessor sample and the pending samples."""
    assert host_run.returncode == 0 and "fbank_stream_host: ok" in host_run.stdout, host_run.stdout[-4000:] + host_run.stderr[-2000:]


def test_first_pushes_of_one_shift(host_run):
    """the reference needs frame_len = 400 samples, then emits one frame per shift: no warm-up skip"""
    m = re.search(r"^first_pushes(( \d+)+)$", host_run.stdout, flags=re.M)
    assert m, host_run.stdout[-2000:]
    assert [int(v) for v in m.group(1).split()] == [0, 0, 1, 1, 1]


def test_errors_without_a_device():
    """NULL handles and zero sizes are refused before any device is touched; id out of range / an id twice / an over-long chunk are the plan
    header's refusals (checked in test_bank_bookkeeping_on_the_host: codes 1, 1, 2 = INVALID_ARG, INVALID_ARG, CAPACITY)"""
    from mel_spec_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    u32 = (C.c_uint32 * 2)(0, 1)
    f32 = (C.c_float * 8)()
    u64 = (C.c_uint64 * 2)()
    assert L.melspec_fbank_stream_create(None, None, 4, 160) == _lib.ERR_INVALID_ARG and "out is NULL" in _lib.last_error()
    assert L.melspec_fbank_stream_create(C.byref(h), None, 0, 160) == _lib.ERR_INVALID_ARG and "must be > 0" in _lib.last_error()
    assert L.melspec_fbank_stream_create(C.byref(h), None, 4, 0) == _lib.ERR_INVALID_ARG and "must be > 0" in _lib.last_error()
    assert L.melspec_fbank_stream_create(C.byref(h), None, 4, 160) == _lib.ERR_INVALID_ARG and "fbank is NULL" in _lib.last_error()
    assert not h.value
    calls = [
        lambda: L.melspec_fbank_stream_reset(None, None, 0),
        lambda: L.melspec_fbank_stream_push_host(None, u32, f32, 0, u32, 1, f32, 8, u32),
        lambda: L.melspec_fbank_stream_push_device(None, u32, None, 0, None, u32, 1, None, None, u32, None),
        lambda: L.melspec_fbank_stream_stats_host(None, u32, 1, f32, u64),
        lambda: L.melspec_fbank_stream_stats_device(None, u32, 1, None, u64, None),
    ]
    # the handle is looked at first: before n == 0, before NULL ids / lens / samples / means, before the dtype codes
    assert L.melspec_fbank_stream_create(None, None, 0, 0) == _lib.ERR_INVALID_ARG and "out is NULL" in _lib.last_error()
    calls += [
        lambda: L.melspec_fbank_stream_push_host(None, None, None, 0, None, 0, None, 0, None),
        lambda: L.melspec_fbank_stream_push_host(None, None, None, 7, None, 1, None, 0, None),
        lambda: L.melspec_fbank_stream_push_device(None, None, None, 1, None, None, 1, None, None, None, None),
        lambda: L.melspec_fbank_stream_stats_host(None, None, 0, None, None),
        lambda: L.melspec_fbank_stream_stats_host(None, None, 1, None, None),
        lambda: L.melspec_fbank_stream_stats_device(None, None, 1, None, None, None),
    ]
    # a handle of another bank (the NeMo bank's tag in its first word) reads as NULL
    other = (C.c_uint32 * 16)(0x4D4C424E)
    calls += [
        lambda: L.melspec_fbank_stream_reset(other, None, 0),
        lambda: L.melspec_fbank_stream_push_host(other, u32, f32, 0, u32, 1, f32, 8, u32),
        lambda: L.melspec_fbank_stream_stats_host(other, u32, 1, f32, u64),
    ]
    for k, call in enumerate(calls):
        assert call() == _lib.ERR_INVALID_ARG, k
        assert "fbank stream bank is NULL" in _lib.last_error(), (k, _lib.last_error())
    for h_bad in (None, other):
        assert L.melspec_fbank_stream_frames_after(h_bad, 0, 400) == 0
        assert not L.melspec_fbank_stream_input_ptr(h_bad, 0)
        assert L.melspec_fbank_stream_supports_io(h_bad, 0, 0) == 0
        L.melspec_fbank_stream_destroy(h_bad)
    assert other[0] == 0x4D4C424E and not any(other[i] for i in range(1, 16))


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
    assert hasattr(M, "FbankStreamBank")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------

def _sources(jfk, n_streams=7, n=24000):
    return [np.ascontiguousarray(jfk[(7919 * s) % 60000:][:n] * np.float32(1.0 + 0.1 * s)) for s in range(n_streams)]


def _drive(bank, src, shift, max_chunk, seed):
    """tests/test_stream.py's _drive for this bank: random-sized chunks (incl. sizes below, at and above a shift and a frame) to a random
    subset of the streams per push; returns every stream's concatenated rows"""
    rng = np.random.default_rng(seed)
    n_streams = len(src)
    pos = [0] * n_streams
    got = [[np.zeros((0, bank.n_mels), np.float32)] for _ in range(n_streams)]
    sizes = [0, 1, shift - 1, shift, shift + 1, 2 * shift, 399, 400, 401, max_chunk]
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
        assert [len(r) for r in res] == want_counts
        for s, r in zip(ids, res):
            got[s].append(r.copy())
            if pos[s] >= len(src[s]):
                live.discard(s)
    return [np.concatenate(g) for g in got]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _left_fold_means(rows):
    """the numpy restatement of the bank's statistics: f64 left fold over the rows in order, / count, cast to f32"""
    s = np.zeros(rows.shape[1], np.float64)
    for r in rows:
        s = s + r.astype(np.float64)
    return (s / rows.shape[0]).astype(np.float32)


CONFIGS = [
    ("default", dict(), 1000, False),
    ("shift_7_5ms", dict(frame_shift_ms=7.5), 517, False),
    ("bins_40", dict(num_mel_bins=40), 1000, False),
    ("runtime_bank", dict(low_freq=100.0, high_freq=7000.0), 700, False),
    ("no_preemphasis", dict(preemphasis=0.0), 1000, False),
    ("linear", dict(use_log_fbank=False), 1000, False),
    ("int16", dict(), 640, True),
]


def _oracle_cfg(oracle, kw, apply_cmn):
    oc = oracle.fbank_default_config()
    for k, v in kw.items():
        setattr(oc, k, int(v) if isinstance(v, bool) else v)
    oc.apply_cmn = int(apply_cmn)
    return oc


@pytest.mark.gpu
@pytest.mark.parametrize("name,kw,max_chunk,s16", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_gpu_random_chunks_rows_and_means(gpu, oracle, jfk, name, kw, max_chunk, s16):
    """7 streams of 24 000 JFK samples, each scaled differently, two seeds (two different cuts of the same sources): rows bit-equal to the
    batch call of an apply_cmn = 0 twin on the concatenation and between the cuts, within TOL of the oracle; means bit-equal between
    the cuts, to the numpy left fold over the bank's own rows and between stats_host and stats_device, within TOL of the oracle's f64
    column mean; rows - means within 2 TOL of the oracle's CMN output (rows and means are each within TOL; the oracle's own f32 fold
    is 4.8e-6 from the f64 mean on these slices)."""
    src = _sources(jfk)
    if s16:
        q = [np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16) for x in src]
        src, as_f32 = q, [x.astype(np.float32) * np.float32(2.0 ** -15) for x in q]
    else:
        as_f32 = src
    fb = gpu.Fbank(gpu.FbankConfig(apply_cmn=True, **kw))
    twin = gpu.Fbank(gpu.FbankConfig(apply_cmn=False, **kw))
    assert fb.uses_fast_path
    shift = fb.config.frame_shift_samples()
    oc0, oc1 = _oracle_cfg(oracle, kw, False), _oracle_cfg(oracle, kw, True)
    runs = []
    for seed in (11, 12):
        bank = gpu.FbankStreamBank(fb, len(src), max_chunk)
        rows = _drive(bank, src, shift, max_chunk, seed)
        means, counts = bank.stats(list(range(len(src))))
        d_means = gpu.DeviceBuffer(means.nbytes)
        counts_d = bank.stats_device(list(range(len(src))), d_means.ptr)
        means_d = d_means.download(means.shape)
        d_means.free(); bank.close()
        assert np.array_equal(counts, counts_d) and np.array_equal(_bits(means), _bits(means_d))
        runs.append((rows, means, counts))
    worst = worst_mean = worst_cmn = 0.0
    for s in range(len(src)):
        (r1, m1, c1), (r2, m2, _) = runs
        batch = twin.compute(as_f32[s])
        want = oracle.fbank_compute(as_f32[s], oc0)
        assert r1[s].shape == batch.shape == want.shape and int(c1[s]) == want.shape[0]
        assert np.array_equal(_bits(r1[s]), _bits(batch)), (name, s, "rows differ from the batch call")
        assert np.array_equal(_bits(r1[s]), _bits(r2[s])) and np.array_equal(_bits(m1[s]), _bits(m2[s])), (name, s, "another cut, other bits")
        assert np.array_equal(_bits(m1[s]), _bits(_left_fold_means(r1[s]))), (name, s, "means are not the left fold of the rows")
        tol = TOL if kw.get("use_log_fbank", True) else 1e-4 * max(1.0, float(np.abs(want).max()))
        d = float(np.abs(r1[s] - want).max()); worst = max(worst, d / tol)
        dm = float(np.abs(m1[s] - want.astype(np.float64).mean(axis=0)).max()); worst_mean = max(worst_mean, dm / tol)
        dc = float(np.abs((r1[s] - m1[s]) - oracle.fbank_compute(as_f32[s], oc1)).max()); worst_cmn = max(worst_cmn, dc / (2 * tol))
    print(f"{name}: rows {worst:.3f} means {worst_mean:.3f} rows - means {worst_cmn:.3f} (fractions of their bounds)")
    assert worst <= 1.0 and worst_mean <= 1.0 and worst_cmn <= 1.0
    fb.close(); twin.close()


@pytest.mark.gpu
@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
def test_gpu_predecessor_sample(gpu, oracle, jfk, poison):
    """src/fbank.rs:177-181: a frame's first sample is pre-emphasised with the sample in front of it.  A non-finite value at sample
    shift - 1 is inside frame 0 and the predecessor of frame 1 (NaN * 0 = NaN: the whole frame, every bin floored), and no part of
    frame 2.  Pushed as 400 + 160 + 160 the poisoned sample is the predecessor of a push's first frame -- the frame a bank that ran
    its pushes as plain clips would get wrong.  After a reset the stream's frame 0 has no predecessor, whatever the slot held."""
    fb = gpu.Fbank(gpu.FbankConfig())
    oc = _oracle_cfg(oracle, {}, False)
    shift = 160
    clean = np.ascontiguousarray(jfk[20000:20720])
    bad = clean.copy(); bad[shift - 1] = poison
    bank = gpu.FbankStreamBank(fb, 3, 400)
    got = [[], []]
    for lo, hi in ((0, 400), (400, 560), (560, 720)):
        a, b = bank.push([0, 1], [clean[lo:hi], bad[lo:hi]])
        got[0].append(a.copy()); got[1].append(b.copy())
    c, p = np.concatenate(got[0]), np.concatenate(got[1])
    want = oracle.fbank_compute(bad, oc)
    assert c.shape == p.shape == want.shape == (3, 80)
    ulps4 = 4 * 2.0 ** -20                                               # four f32 ulps at 15.94: the logarithm's last places
    assert np.abs(want[:2] - FLOOR_ROW).max() <= ulps4                   # the reference's own rows: frames 0 and 1 floored
    assert np.isfinite(p).all() and np.abs(p[:2] - FLOOR_ROW).max() <= ulps4, "the predecessor of a push's first frame did not reach it"
    assert np.array_equal(_bits(p[2]), _bits(c[2])) and np.abs(c - oracle.fbank_compute(clean, oc)).max() <= TOL
    # reset, then clean data: frame 0 is the oracle's
    fresh = np.ascontiguousarray(jfk[30000:30400])
    bank.reset([1])
    r = bank.push([1], [fresh])[0]
    assert r.shape == (1, 80) and np.abs(r - oracle.fbank_compute(fresh, oc)).max() <= TOL
    assert np.array_equal(_bits(r), _bits(bank.push([2], [fresh])[0]))   # ... and that of a stream that never held anything
    # the poisoned value as the very last sample before the reset: a stale carry would poison frame 0
    tail = jfk[40000:40500].copy(); tail[-1] = poison                    # (a copy: jfk is the session's)
    bank.push([1], [tail[:400]]); bank.push([1], [tail[400:]])
    bank.reset([1])
    r2 = bank.push([1], [fresh])[0]
    assert np.array_equal(_bits(r2), _bits(r))
    means, counts = bank.stats([1])
    assert counts[0] == 1 and np.array_equal(_bits(means[0]), _bits(r[0]))       # the sums were reset with the history
    bank.close(); fb.close()


@pytest.mark.gpu
def test_gpu_past_one_grid_trip_device_pushes(gpu, oracle, jfk):
    """2 500 streams -- more than 256 CUs x 8 waves -- each fed one of 5 scaled sources, three pushes of 401, 159 and 160 samples written
    at input_ptr and pushed with caller-placed row offsets into fenced buffers: every row of every stream is bit-equal to its source's
    batch rows and nothing outside the rows is written.  reset([2]) leaves stream 3's state intact."""
    from mel_spec_amd import _lib
    n_streams, nm = 2500, 80
    fb = gpu.Fbank(gpu.FbankConfig())
    twin = gpu.Fbank(gpu.FbankConfig(apply_cmn=False))
    srcs = [np.ascontiguousarray(jfk[(7919 * s) % 60000:][:1040] * np.float32(1.0 + 0.1 * s)) for s in range(5)]
    want = [twin.compute(x) for x in srcs]                # 720 samples: 3 rows; 880: 4; 1040: 5
    bank = gpu.FbankStreamBank(fb, n_streams, 401)
    ids = np.arange(n_streams, dtype=np.uint32)
    p0 = bank.input_ptr(0)
    slot = bank.input_ptr(1) - p0
    assert slot > 0 and p0 % 16 == 0 and slot % 16 == 0
    # rows of stream s at (s * 3 + 1) * nm floats: a row of fence in front of the first stream's rows, two behind every stream's row
    FENCE = np.float32(-777.0)
    out = gpu.DeviceBuffer((n_streams * 3 + 1) * nm * 4)
    offs = (np.arange(n_streams, dtype=np.uint64) * 3 + 1) * nm
    pos, emitted = 0, 0
    h2d = _lib.lib().melspec_memcpy_h2d
    for n, rows in ((401, 1), (159, 1), (160, 1)):       # 401, 560, 720 samples: one more frame each
        chunks = [np.ascontiguousarray(x[pos:pos + n]) for x in srcs]
        for s in range(n_streams):                        # the producer writes the chunk -- and nothing else -- into the stream's slot
            c = chunks[s % 5]
            assert h2d(C.c_void_p(p0 + s * slot), c.ctypes.data_as(C.c_void_p), c.nbytes) == 0
        out.upload(np.full((n_streams * 3 + 1) * nm, FENCE, np.float32))
        fr = bank.push_device(ids, np.full(n_streams, n, np.uint32), out.ptr, out_offsets=offs)
        assert (fr == rows).all()
        got = out.download((n_streams * 3 + 1, nm))
        for s in range(5):
            mine = got[1:].reshape(n_streams, 3, nm)[s::5]
            assert np.array_equal(_bits(mine[:, :rows]), np.broadcast_to(_bits(want[s][emitted:emitted + rows]), (mine.shape[0], rows, nm))), (n, s)
            assert (mine[:, rows:] == FENCE).all(), (n, s)
        assert (got[0] == FENCE).all()
        pos += n; emitted += rows
    means, counts = bank.stats(ids)
    assert (counts == 3).all()
    for s in range(5):
        assert (_bits(means[s::5]) == _bits(_left_fold_means(want[s][:3]))).all()
    # a reset stream starts over; its neighbour continues
    bank.reset([2])
    a, b = bank.push([2, 3], [srcs[2][:400], srcs[3][720:880]])
    assert np.array_equal(_bits(a), _bits(want[2][:1])) and np.array_equal(_bits(b), _bits(want[3][3:4]))
    out.free(); bank.close(); fb.close(); twin.close()


@pytest.mark.gpu
def test_gpu_unsupported_objects(gpu, oracle, jfk):
    """an object off the fused path is refused at create; melspec_fbank_use_generic after create makes the next push UNSUPPORTED and the
    push after switching back continues the stream; refused pushes (id out of range, an id twice, an over-long chunk) change nothing"""
    from mel_spec_amd import _lib
    L = _lib.lib()
    slow = gpu.Fbank(gpu.FbankConfig(frame_length_ms=30.0))              # 480-sample frames: the generic path
    assert not slow.uses_fast_path
    h = C.c_void_p()
    assert L.melspec_fbank_stream_create(C.byref(h), slow._h, 4, 160) == _lib.ERR_UNSUPPORTED and not h.value
    assert "frame_length = 480" in _lib.last_error()
    slow.close()
    fb = gpu.Fbank(gpu.FbankConfig(apply_cmn=False))
    x = np.ascontiguousarray(jfk[5000:6000])
    want = fb.compute(x)
    bank = gpu.FbankStreamBank(fb, 2, 600)
    a = bank.push([1], [x[:500]])[0]
    fb.use_generic(True)
    with pytest.raises(gpu.HipError) as e:
        bank.push([1], [x[500:]])
    assert e.value.code == _lib.ERR_UNSUPPORTED and "generic" in str(e.value)
    fb.use_generic(False)
    b = bank.push([1], [x[500:]])[0]                                      # the refused push left the stream where it was
    assert np.array_equal(_bits(np.concatenate([a, b])), _bits(want))
    # the refusals of a push through the ABI: the codes melspec_stream_push_host returns for them, the stream untouched
    x2 = np.ascontiguousarray(jfk[7000:7800])
    a = bank.push([0], [x2[:300]])[0]
    for ids, chunks, code in (([2], [x2[:10]], _lib.ERR_INVALID_ARG), ([0, 0], [x2[:10], x2[:10]], _lib.ERR_INVALID_ARG),
                              ([1, 0], [x2[:10], x2[:601]], _lib.ERR_CAPACITY)):
        with pytest.raises(gpu.HipError) as e:
            bank.push(ids, chunks)
        assert e.value.code == code, (ids, str(e.value))
    b = bank.push([0], [x2[300:800]])[0]
    assert a.shape[0] == 0 and np.array_equal(_bits(b), _bits(fb.compute(x2)))
    bank.close(); fb.close()


@pytest.mark.gpu
def test_gpu_reset_with_a_bad_id_resets_nothing(gpu, oracle, jfk):
    """melspec_fbank_stream_reset checks every id before it touches anything: reset([0, 7]) on a bank of two streams is INVALID_ARG and
    stream 0, listed in front of the bad id, goes on where it was -- both streams' rows are the batch call's rows of all six shifts,
    bit for bit."""
    from mel_spec_amd import _lib
    fb = gpu.Fbank(gpu.FbankConfig(apply_cmn=False))
    bank = gpu.FbankStreamBank(fb, 2, 400)
    src = [np.ascontiguousarray(jfk[20000:20000 + 960]), np.ascontiguousarray(jfk[41000:41000 + 960])]
    got = [[], []]

    def push_shifts(first):
        for k in range(first, first + 3):
            for i, r in enumerate(bank.push([0, 1], [s[k * 160:(k + 1) * 160] for s in src])):
                got[i].append(r)

    push_shifts(0)
    with pytest.raises(gpu.HipError) as e:
        bank.reset([0, 7])
    assert e.value.code == _lib.ERR_INVALID_ARG and "out of range" in str(e.value)
    push_shifts(3)
    for i in range(2):
        want = fb.compute(src[i])
        mine = np.concatenate(got[i])
        assert want.shape[0] == 4 and mine.shape == want.shape and np.array_equal(_bits(mine), _bits(want)), i
    bank.close(); fb.close()
