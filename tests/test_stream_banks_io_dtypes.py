"""f16 / bf16 rows out of the Kaldi fbank's and the NeMo / Parakeet frontend's stream banks (melspec_fbank_stream_*_io,
melspec_blm_stream_*_io): the pushes -- and the NeMo bank's finish -- with typed ends.

The yardstick is a twin bank and it is exact: a bank driven through the _io calls must emit, push by push (for NeMo through finish),
the frames_out of a twin bank -- a second object of the same config -- driven through the existing f32 calls on
`chunk.astype(float32) * float32(2**-15)`, and rows that are round_to(the twin's rows, out) as bits, with equal NaN masks; after the last
call the two banks' stats are array_equal (Kaldi: means and counts; NeMo: mean, inv_std and counts): the statistics are folds over the f32
rows and never see the rounded ones.  No tolerance anywhere but against the oracle, where the gates are those tests/test_fbank_io_dtypes.py
and tests/test_blm_io_dtypes.py use for 16-bit rows (the path's gate + half a unit in the last place of the type at the expected element's
magnitude; imported, not restated) -- which needs the oracle's rows to be finite f16 values, checked here on the CPU.

Every output, host or device, is the middle of an allocation filled with the type's sentinel with a guard band on each side
(tests/test_stream_io_dtypes.py: HostFence, DevFence); device pushes use odd element offsets with gaps between the entries.  Bands and gaps
must still hold the sentinel afterwards and every element of the output proper must have been written; after a refused call all of it is
the sentinel.

Shapes: 7 streams of 8000 + 37 s int16 samples, max_chunk 2000, the random schedule of tests/test_stream_io_dtypes.py (chunk sizes 0, 1,
159 / 160 / 161, 399 / 400 / 401, ... to random subsets of the streams, chunks staged at odd elements); the Kaldi default bank (80 bins,
shift 160), a 40-bin Kaldi object (it streams but is outside the batch _io calls' condition: typed rows exist on every geometry a bank
can be created on), NeMo at 80 and 128 mels, centred and not, in f64 and MELSPEC_PRECISION_F32.  The twin's run of a config is made once
and shared by the tests that need it."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_blm_io_dtypes import TOL as BLM_TOL, half_ulp
from test_fbank_io_dtypes import TOL as FBANK_TOL
from test_fbank_stream import _oracle_cfg
from test_io_dtypes import (ERR_CAPACITY, ERR_INVALID_ARG, OUT_BF16, OUT_F16, OUT_F32, OUT_NP, PCM_F32, PCM_S16, round_to, s16_speech, to_f32,
                            to_f64)
from test_stream_io_dtypes import PCM_NP, DevFence, HostFence, gapped, gapped_rows, schedule, sources

u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
SYMBOLS = ["melspec_fbank_stream_supports_io", "melspec_fbank_stream_push_host_io", "melspec_fbank_stream_push_device_io",
           "melspec_blm_stream_supports_io", "melspec_blm_stream_push_host_io", "melspec_blm_stream_push_device_io",
           "melspec_blm_stream_finish_host_io", "melspec_blm_stream_finish_device_io"]
TYPED = [(PCM_F32, OUT_F16), (PCM_F32, OUT_BF16), (PCM_S16, OUT_F16), (PCM_S16, OUT_BF16)]        # every (pcm, out) pair with out != F32
N_STREAMS, MAX_CHUNK, SEED = 7, 2000, 21
F16_MAX = 65504.0                               # the oracle's rows must be finite f16 values for the half-ulp term to mean anything

# name -> (kind, config, precision mode)
BANKS = {
    "kaldi_80": ("kaldi", dict(), None),
    "kaldi_40": ("kaldi", dict(num_mel_bins=40), None),
    "nemo_80_f64": ("nemo", dict(preemphasis=0.97), "f64"),
    "nemo_80_f32": ("nemo", dict(preemphasis=0.97), "f32"),
    "nemo_128_f64": ("nemo", dict(n_mels=128, preemphasis=0.97), "f64"),
    "nemo_128_f32": ("nemo", dict(n_mels=128, preemphasis=0.97), "f32"),
    "nemo_80_nocenter_f64": ("nemo", dict(center=False, preemphasis=0.97), "f64"),
    "nemo_80_nocenter_f32": ("nemo", dict(center=False, preemphasis=0.97), "f32"),
    "nemo_128_nocenter_f64": ("nemo", dict(n_mels=128, center=False), "f64"),
    "nemo_128_nocenter_f32": ("nemo", dict(n_mels=128, center=False), "f32"),
}
THREE = ["kaldi_80", "nemo_80_f64", "nemo_128_nocenter_f32"]      # one of each fold kernel, both NeMo precisions, both origins


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _u32(a):
    return np.ascontiguousarray(a, np.uint32)


# ---- the calls ---------------------------------------------------------------------------------------------------------------------

class Bank:
    """a bank over an object of its own; the typed calls go through the C ABI into fenced outputs, the f32 calls through the Python mirror.
    Rows are handled flat, entry after entry, as the calls lay them out (Kaldi [frame][bin], NeMo [mel][frame] per entry)."""

    def __init__(self, gpu, name, n_streams=N_STREAMS, max_chunk=MAX_CHUNK):
        self.kind, kw, mode = BANKS[name]
        self.gpu, self.lib, self.n_streams, self.max_chunk = gpu, gpu._lib.lib(), n_streams, max_chunk
        if self.kind == "kaldi":
            self.obj, self.P = gpu.Fbank(gpu.FbankConfig(**kw)), "melspec_fbank_stream_"
        else:
            self.obj, self.P = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw)), "melspec_blm_stream_"
            self.obj.set_precision(mode)
            assert self.obj.precision == mode
        self.bank = None
        self.fresh()

    def fresh(self):
        """a new bank on the same object"""
        if self.bank is not None:
            self.bank.close()
        self.bank = (self.gpu.FbankStreamBank if self.kind == "kaldi" else self.gpu.BlmStreamBank)(self.obj, self.n_streams, self.max_chunk)
        self.h, self.nm = self.bank._h, self.bank.n_mels
        return self

    def close(self):
        self.bank.close(); self.obj.close()          # both idempotent

    def fn(self, name):
        return getattr(self.lib, self.P + name)

    def counts(self, ids, lens):
        """rows the call will emit per entry (lens None: a finish)"""
        if lens is None:
            return [self.bank.finish_frames(int(s)) for s in ids]
        return [self.bank.frames_after(int(s), int(n)) for s, n in zip(ids, lens)]

    def stats(self):
        return self.bank.stats(list(range(self.n_streams)))

    def plain(self, ids, chunks):
        """the existing f32 call (chunks None: finish) -> (frames_out, bits of the f32 rows)"""
        res = self.bank.finish(ids) if chunks is None else self.bank.push(ids, [np.ascontiguousarray(c, np.float32) for c in chunks])
        frames = np.array([r.size // self.nm for r in res], np.uint32)
        flat = np.concatenate([np.ascontiguousarray(r, np.float32).reshape(-1) for r in res])
        return frames, flat.view(np.uint32)

    def host_io(self, ids, chunks, pcm, out, expect=0, cap=None):
        """push_host_io (chunks None: finish_host_io) -> (frames_out, bits of the rows) -- or, expect != 0, asserts the status and that
        output and frames_out are untouched"""
        ids = _u32(ids)
        lens = None if chunks is None else _u32([len(c) for c in chunks])
        if cap is None:
            cap = sum(self.counts(ids, lens)) * self.nm
        f = HostFence(cap, out if out in OUT_NP else OUT_F16)
        frames = np.full(len(ids), 0xABCD, np.uint32)
        if chunks is None:
            rc = self.fn("finish_host_io")(self.h, ids.ctypes.data_as(u32p), len(ids), f.ptr, out, cap, frames.ctypes.data_as(u32p))
        else:
            dt = PCM_NP.get(pcm, np.int16)          # an unknown code: the call must fail before it looks at the buffers
            flat = np.ascontiguousarray(np.concatenate(chunks), dt)
            flat = flat if flat.size else np.zeros(1, dt)
            rc = self.fn("push_host_io")(self.h, ids.ctypes.data_as(u32p), _vp(flat), pcm, lens.ctypes.data_as(u32p), len(ids), f.ptr, out, cap,
                                         frames.ctypes.data_as(u32p))
        assert rc == expect, (rc, expect, self.lib.melspec_last_error())
        if expect:
            assert f.untouched() and np.all(frames == 0xABCD), "a refused call wrote into its output"
            return None
        assert int(frames.sum()) * self.nm == cap
        return frames, f.bits(cap)

    def dev_io(self, fence, ids, chunks, pcm, out, gaps=True, expect=0, at_input_ptr=False):
        """push_device_io (chunks None: finish_device_io) into `fence`: the chunks in a device buffer with filler in gaps of 1-2 elements
        (at_input_ptr: d_chunks == NULL, the f32 chunks written at input_ptr), the rows at odd offsets with gaps (gaps False: packed,
        h_out_offsets == NULL) -> (frames_out, bits of the rows, entry after entry)"""
        ids = _u32(ids)
        lens = None if chunks is None else _u32([len(c) for c in chunks])
        counts = self.counts(ids, lens)
        sizes = [k * self.nm for k in counts]
        oo, total = gapped_rows(counts, self.nm) if gaps else (np.cumsum([0] + sizes[:-1]).astype(np.uint64), sum(sizes))
        assert total <= fence.n
        fence.arm(out if out in OUT_NP else OUT_F16)
        frames = np.full(len(ids), 0xABCD, np.uint32)
        oo_p = oo.ctypes.data_as(u64p) if gaps else None
        d = None
        if chunks is None:
            rc = self.fn("finish_device_io")(self.h, ids.ctypes.data_as(u32p), len(ids), C.c_void_p(fence.ptr), out, oo_p, frames.ctypes.data_as(u32p), None)
        elif at_input_ptr:
            for s, c in zip(ids, chunks):
                x = np.ascontiguousarray(c, np.float32)
                assert x.size == 0 or self.lib.melspec_memcpy_h2d(C.c_void_p(self.bank.input_ptr(int(s))), _vp(x), x.nbytes) == 0
            rc = self.fn("push_device_io")(self.h, ids.ctypes.data_as(u32p), None, pcm, None, lens.ctypes.data_as(u32p), len(ids), C.c_void_p(fence.ptr), out,
                                           oo_p, frames.ctypes.data_as(u32p), None)
        else:
            flat, so = gapped(chunks, PCM_NP.get(pcm, np.int16))
            d = self.gpu.DeviceBuffer(flat.nbytes); d.upload(flat)
            rc = self.fn("push_device_io")(self.h, ids.ctypes.data_as(u32p), C.c_void_p(d.ptr), pcm, so.ctypes.data_as(u64p), lens.ctypes.data_as(u32p),
                                           len(ids), C.c_void_p(fence.ptr), out, oo_p, frames.ctypes.data_as(u32p), None)
        if d is not None:
            d.free()                                 # the launches have completed on return
        assert rc == expect, (rc, expect, self.lib.melspec_last_error())
        if expect:
            assert fence.untouched() and np.all(frames == 0xABCD), "a refused call wrote into its output"
            return None
        assert list(frames) == counts
        return frames, np.concatenate(fence.rows(oo, sizes))


@pytest.fixture
def banks(gpu):
    """Bank(...) factory; every bank is closed in front of its object at teardown, also when the test failed"""
    made = []

    def make(name, n_streams=N_STREAMS, max_chunk=MAX_CHUNK):
        made.append(Bank(gpu, name, n_streams, max_chunk))
        return made[-1]

    yield make
    for b in reversed(made):
        b.close()


def drive(b, src, pushes, call):
    """the whole schedule and, for a NeMo bank, a finish of all streams in two calls; call(k, ids, chunks or None) -> (frames_out, bits)"""
    pos, res = [0] * len(src), []
    for ids, lens in pushes:
        chunks = [src[s][pos[s]:pos[s] + n] for s, n in zip(ids, lens)]
        for s, n in zip(ids, lens):
            pos[s] += n
        res.append(call(len(res), ids, chunks))
    assert pos == [len(x) for x in src]
    if b.kind == "nemo":
        order = list(range(len(src)))
        for ids in (order[:3], order[3:]):
            res.append(call(len(res), ids, None))
    return res


def same_rows(got, twin32, out, what):
    """got: bits of the typed rows; twin32: bits of the twin's f32 rows.  NaN exactly where the twin has one, the rounded bits elsewhere."""
    want = round_to(twin32, out)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan_g, nan_w = np.isnan(to_f64(got, out)), np.isnan(to_f64(want, out))
    assert np.array_equal(nan_g, nan_w), f"{what}: NaN at {int(nan_g.sum())} elements, the twin at {int(nan_w.sum())}"
    diff = (got != want) & ~nan_w
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ from the twin's (rounded) bits, first at " \
                           f"{int(np.argmax(diff))}: {got[np.argmax(diff)]:#x} != {want[np.argmax(diff)]:#x}"


def same_pushes(got, want, outs, what):
    """outs: the row type of every call, or one for all"""
    assert len(got) == len(want)
    for k, ((fg, bg), (fw, bw)) in enumerate(zip(got, want)):
        assert np.array_equal(fg, fw), f"{what}: call {k}: frames_out {fg} != the twin's {fw}"
        same_rows(bg, bw, outs[k] if isinstance(outs, list) else outs, f"{what}: call {k}")


def same_stats(b, twin_stats, what):
    got = b.stats()
    assert len(got) == len(twin_stats)
    for g, w in zip(got, twin_stats):
        assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32 if g.dtype == np.float32 else g.dtype), w.view(np.uint32 if w.dtype == np.float32 else w.dtype)), \
            f"{what}: the statistics are not the f32-driven twin's"


@pytest.fixture(scope="module")
def twins(gpu, jfk):
    """twins(name) -> (s16 sources, their f32 conversions, the schedule, the twin's (frames_out, f32 bits) per call, the twin's final
    stats): the twin bank of a config driven through the existing f32 calls, once per module"""
    s16 = sources(jfk, N_STREAMS)
    f32 = [to_f32(x) for x in s16]
    pushes = schedule([len(x) for x in s16], MAX_CHUNK, SEED)
    made = {}

    def get(name):
        if name not in made:
            t = Bank(gpu, name)
            want = drive(t, f32, pushes, lambda k, ids, chunks: t.plain(ids, chunks))
            for _, bits in want:
                bits.setflags(write=False)
            made[name] = (want, t.stats())
            t.close()
            assert sum(int(f.sum()) for f, _ in made[name][0]) > N_STREAMS * 40
        return (s16, f32, pushes) + made[name]

    return get


def fence_for(gpu, n_streams=N_STREAMS, max_chunk=MAX_CHUNK):
    return DevFence(gpu, n_streams * (max_chunk // 160 + 4) * 128 + 16 * n_streams + 64)


# ---- 1. twin equality --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("name", list(BANKS))
def test_twin_equality(gpu, banks, twins, name, form):
    """for every (pcm, out) pair with out != F32 a fresh bank through the _io calls -- the host forms, or the device forms with gapped
    chunks and rows at odd offsets with gaps -- against the twin: frames_out, rows and the final stats"""
    s16, f32, pushes, want, want_stats = twins(name)
    b = banks(name)
    fence = fence_for(gpu) if form == "device" else None
    for pcm, out in TYPED:
        assert b.fresh().bank.supports_io(pcm, out)
        if form == "host":
            call = lambda k, ids, chunks: b.host_io(ids, chunks, pcm, out)
        else:
            call = lambda k, ids, chunks: b.dev_io(fence, ids, chunks, pcm, out)
        got = drive(b, s16 if pcm == PCM_S16 else f32, pushes, call)
        same_pushes(got, want, out, f"{name} {form} ({pcm}, {out})")
        same_stats(b, want_stats, f"{name} {form} ({pcm}, {out})")
    if fence:
        fence.buf.free()


# ---- 2. mixed use ------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", THREE)
def test_mixed_use_of_one_bank(gpu, banks, twins, name):
    """one bank, call k: the existing f32 call, a typed host call, a typed device call (with chunks in a device buffer or at input_ptr) in
    turn, the row type cycling f32 / f16 / bf16 on the same streams: every call's rows are the twin's (rounded where typed) and the
    final stats are the twin's -- no scratch or plan leaks between row types"""
    s16, f32, pushes, want, want_stats = twins(name)
    b = banks(name)
    fence = fence_for(gpu)
    outs = [(OUT_F32, OUT_F16, OUT_BF16)[(k + k // 3) % 3] for k in range(len(want))]

    def call(k, ids, chunks):
        out, how = outs[k], k % 4
        if how == 0 and out == OUT_F32:
            return b.plain(ids, chunks)
        if how == 1:
            return b.host_io(ids, chunks, PCM_F32, out)
        if how == 2 and chunks is not None:
            return b.dev_io(fence, ids, chunks, PCM_F32, out, gaps=False, at_input_ptr=True)
        return b.dev_io(fence, ids, chunks, PCM_F32, out)

    got = drive(b, f32, pushes, call)
    assert {OUT_F32, OUT_F16, OUT_BF16} <= set(outs)
    same_pushes(got, want, outs, f"{name} mixed")
    same_stats(b, want_stats, f"{name} mixed")
    fence.buf.free()


# ---- 3. fences: neighbouring entries in one 4-byte word ----------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["nemo_80_f64", "nemo_128_f32", "kaldi_40"])
def test_entries_that_share_a_word(gpu, banks, jfk, name, out):
    """three entries back to back from element 1 on, the NeMo ones with 1, 3 and 1 columns (every mel row of the middle entry starts at an odd
    element): the last element of an entry and the first of the next lie in one 4-byte word, as do the sentinel in front of the first and
    behind the last.  Rows are the twin's, everything else is still the sentinel.  (Tests 1, 2 and 7 fence every other output.)"""
    b, t = banks(name, 3, 800), banks(name, 3, 800)
    lens = [200, 520, 200] if b.kind == "nemo" else [400, 720, 560]        # NeMo centred: 1, 3, 1 columns; Kaldi: 1, 3, 2 rows
    src = [s16_speech(jfk, s, n) for s, n in enumerate(lens)]
    counts = b.counts([0, 1, 2], lens)
    assert counts == ([1, 3, 1] if b.kind == "nemo" else [1, 3, 2])
    sizes = [k * b.nm for k in counts]
    oo = (1 + np.cumsum([0] + sizes[:-1])).astype(np.uint64)
    fence = DevFence(gpu, 4096).arm(out)
    flat = np.concatenate(src)
    d = gpu.DeviceBuffer(flat.nbytes); d.upload(flat)
    frames = np.zeros(3, np.uint32)
    ids = _u32([0, 1, 2])
    rc = b.fn("push_device_io")(b.h, ids.ctypes.data_as(u32p), C.c_void_p(d.ptr), PCM_S16, None, _u32(lens).ctypes.data_as(u32p), 3, C.c_void_p(fence.ptr), out,
                                oo.ctypes.data_as(u64p), frames.ctypes.data_as(u32p), None)
    assert rc == 0, b.lib.melspec_last_error()
    d.free()
    fw, bw = t.plain([0, 1, 2], [to_f32(x) for x in src])
    assert list(frames) == list(fw) == counts
    same_rows(np.concatenate(fence.rows(oo, sizes)), bw, out, f"{name} out {out}")
    same_stats(b, t.stats(), name)
    fence.buf.free()


# ---- 4. more entries than compute units --------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", THREE)
def test_more_entries_than_compute_units(gpu, banks, jfk, name):
    """one push of 300 streams with 560 samples each (one to three rows per stream): more fold workgroups than the 256 CUs.  Typed device
    push, packed, against the twin's push; then the stats"""
    n = 300
    b, t = banks(name, n, 560), banks(name, n, 560)
    base = sources(jfk, 5, 560)
    src = [base[s % 5][:560] for s in range(n)]
    ids = list(range(n))
    fw, bw = t.plain(ids, [to_f32(x) for x in src])
    assert 1 <= int(fw.min()) and int(fw.max()) <= 3
    fence = DevFence(gpu, n * 3 * b.nm + 64)
    for k, out in enumerate((OUT_F16, OUT_BF16)):
        if k:
            b.fresh()
        fg, bg = b.dev_io(fence, ids, src, PCM_S16, out, gaps=False)
        assert np.array_equal(fg, fw)
        same_rows(bg, bw, out, f"{name} 300 entries out {out}")
        same_stats(b, t.stats(), f"{name} 300 entries out {out}")
    fence.buf.free()


# ---- 5. one long entry -------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", THREE)
def test_one_long_entry(gpu, banks, jfk, name):
    """max_chunk 16000, one stream, one chunk of 16000 samples (about 100 rows) and, for NeMo, the finish: the fold's serial walk over a
    long entry, host and device form, against the twin"""
    b, t = banks(name, 1, 16000), banks(name, 1, 16000)
    x = s16_speech(jfk, 3, 16000)
    want = [t.plain([0], [to_f32(x)])] + ([t.plain([0], None)] if t.kind == "nemo" else [])
    assert 97 <= int(want[0][0][0]) <= 100
    fence = DevFence(gpu, 101 * b.nm + 64)
    for k, (form, out) in enumerate((("host", OUT_F16), ("device", OUT_BF16), ("host", OUT_BF16), ("device", OUT_F16))):
        if k:
            b.fresh()
        call = (lambda ch: b.host_io([0], ch, PCM_S16, out)) if form == "host" else (lambda ch: b.dev_io(fence, [0], ch, PCM_S16, out))
        got = [call([x])] + ([call(None)] if b.kind == "nemo" else [])
        same_pushes(got, want, out, f"{name} long entry {form} out {out}")
        same_stats(b, t.stats(), f"{name} long entry {form} out {out}")
    fence.buf.free()


# ---- 6. non-finite input -----------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", THREE)
def test_nonfinite_input(gpu, banks, jfk, name):
    """one stream with a NaN just before a chunk border and an infinity at the next one (pre-emphasis carries both across the border): the
    typed rows are NaN exactly where the twin's are and its bits elsewhere; so are the statistics (NaN where the twin's are)"""
    b, t = banks(name, 1, 800), banks(name, 1, 800)
    x = to_f32(s16_speech(jfk, 1, 2400)).copy()
    x[799], x[1600] = np.nan, np.inf
    cuts = [x[0:800], x[800:1600], x[1600:2400]] + ([None] if b.kind == "nemo" else [])
    want = [t.plain([0], None if c is None else [c]) for c in cuts]
    want_stats = t.stats()
    # the poison reaches some rows of the twin and not all: as NaN in the NeMo bank; the Kaldi reference floors such a frame (its
    # max(energy, epsilon) drops the NaN: tests/test_fbank_stream.py, test_gpu_predecessor_sample), so there the rows differ from clean ones
    t.fresh()
    y = to_f32(s16_speech(jfk, 1, 2400))
    clean = [t.plain([0], None if c is None else [y[800 * k:800 * k + 800]]) for k, c in enumerate(cuts)]
    hit = np.concatenate([bw != bc for (_, bw), (_, bc) in zip(want, clean)])
    n_nan = sum(int(np.isnan(bw.view(np.float32)).sum()) for _, bw in want)
    assert 0 < int(hit.sum()) < hit.size and (n_nan > 0) == (b.kind == "nemo"), (int(hit.sum()), hit.size, n_nan)
    for k, out in enumerate((OUT_F16, OUT_BF16)):
        if k:
            b.fresh()
        got = [b.host_io([0], None if c is None else [c], PCM_F32, out) for c in cuts]
        same_pushes(got, want, out, f"{name} non-finite out {out}")
        for g, w in zip(b.stats(), want_stats):
            assert np.array_equal(g, w, equal_nan=g.dtype == np.float32), f"{name}: statistics differ from the twin's"


# ---- 7. refusals -------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kaldi_80", "nemo_80_f64"])
def test_refusals(gpu, banks, jfk, name):
    """a bad dtype code, an id listed twice, an over-long chunk, d_chunks == NULL with S16 and, for NeMo, a typed push or finish to an ended
    stream: the code the f32 call gives, a fenced output that is entirely sentinel, frames_out untouched -- and the next valid push goes on
    bit-equal to the twin, which never saw the refused calls.  Host and device forms."""
    b, t = banks(name, 3, 600), banks(name, 3, 600)
    s16 = sources(jfk, 3, 6000)
    fence = DevFence(gpu, 8192)
    pos = [0]

    def go_on(what):
        n = 333
        chunks = [x[pos[0]:pos[0] + n] for x in s16[:2]]
        pos[0] += n
        want = t.plain([0, 1], [to_f32(c) for c in chunks])
        same_pushes([b.host_io([0, 1], chunks, PCM_S16, OUT_F16)], [want], OUT_F16, f"{name}: the push after {what}")

    go_on("nothing")
    c2 = [s16[0][:100], s16[1][:100]]
    long2 = [s16[1][:10], s16[0][:601]]
    refused = [("a bad pcm code", [0, 1], c2, 7, OUT_F16, ERR_INVALID_ARG), ("a bad out code", [0, 1], c2, PCM_S16, 9, ERR_INVALID_ARG),
               ("an id twice", [0, 0], c2, PCM_S16, OUT_BF16, ERR_INVALID_ARG), ("an over-long chunk", [1, 0], long2, PCM_S16, OUT_F16, ERR_CAPACITY)]
    for what, ids, chunks, pcm, out, code in refused:
        b.host_io(ids, chunks, pcm, out, expect=code, cap=4096)
        go_on(what + " (host)")
        b.dev_io(fence, ids, chunks, pcm, out, expect=code)
        go_on(what + " (device)")
    b.dev_io(fence, [0, 1], [to_f32(c) for c in c2], PCM_S16, OUT_F16, gaps=False, expect=ERR_INVALID_ARG, at_input_ptr=True)
    go_on("d_chunks == NULL with S16")
    if b.kind == "nemo":
        x2 = s16[2][:555]
        same_pushes([b.host_io([2], [x2], PCM_S16, OUT_BF16), b.host_io([2], None, PCM_F32, OUT_BF16)],
                    [t.plain([2], [to_f32(x2)]), t.plain([2], None)], OUT_BF16, "stream 2 to its end")
        for chunks in ([s16[2][:50]], None):
            b.host_io([2], chunks, PCM_S16 if chunks else PCM_F32, OUT_F16, expect=ERR_INVALID_ARG, cap=4096)
            assert "finished" in gpu._lib.last_error()
            go_on("a call to an ended stream (host)")
            b.dev_io(fence, [2], chunks, PCM_S16 if chunks else PCM_F32, OUT_F16, expect=ERR_INVALID_ARG)
            go_on("a call to an ended stream (device)")
    same_stats(b, t.stats(), name)
    fence.buf.free()


# ---- 8. oracle sanity --------------------------------------------------------------------------------------------------------------

ORACLE_CUTS = [1000, 1, 399, 2000, 160, 0, 401, 1999, 2000, 40]


def _oracle_input(jfk):
    return s16_speech(jfk, 0, 8000)


def _oracle_rows(oracle, name, x32):
    """-> (the oracle's rows in the bank's layout, f64; the path's gate)"""
    kind, kw, mode = BANKS[name]
    if kind == "kaldi":
        return oracle.fbank_compute(x32, _oracle_cfg(oracle, kw, False)).astype(np.float64), FBANK_TOL
    cfg = oracle.blm_default_config(**kw)
    want, valid = oracle.blm_compute(x32, cfg, True)
    gate = BLM_TOL
    if mode == "f32":           # tests/test_blm_io_dtypes.py: max(TOL, 4 x the distance of the reference's literal f32 arithmetic on the clip)
        lit, _ = oracle.blm_compute(x32, cfg, False)
        gate = max(BLM_TOL, 4.0 * float(np.abs(lit.astype(np.float64) - want).max()))
    return want[:, :valid].astype(np.float64), gate


@pytest.mark.parametrize("name", ["kaldi_80", "nemo_80_f64", "nemo_128_f32"])
def test_oracle_rows_are_f16_values(oracle, jfk, name):
    """the half-ulp term of the gate below is taken at the expected element's magnitude: that needs finite elements inside the f16 range"""
    want, _ = _oracle_rows(oracle, name, to_f32(_oracle_input(jfk)))
    assert want.size > 40 * 40 and np.isfinite(want).all() and float(np.abs(want).max()) < F16_MAX


@pytest.mark.gpu
@pytest.mark.parametrize("out", [OUT_F16, OUT_BF16], ids=["f16", "bf16"])
@pytest.mark.parametrize("name", ["kaldi_80", "nemo_80_f64", "nemo_128_f32"])
def test_typed_rows_against_the_oracle(gpu, banks, oracle, jfk, name, out):
    """one stream, (S16, out), 8000 samples of speech in chunks of mixed sizes (NeMo: and the finish): the concatenated rows against
    oracle.fbank_compute (CMN off) / oracle.blm_compute on the exactly converted samples.  Bound per element: the path's gate + half a unit
    in the last place of the row type at the expected element's magnitude (tests/test_fbank_io_dtypes.py, tests/test_blm_io_dtypes.py)."""
    x = _oracle_input(jfk)
    want, gate = _oracle_rows(oracle, name, to_f32(x))
    assert np.isfinite(want).all() and float(np.abs(want).max()) < F16_MAX
    b = banks(name, 1, 2000)
    pieces, lo = [], 0
    for n in ORACLE_CUTS:
        fr, bits = b.host_io([0], [x[lo:lo + n]], PCM_S16, out)
        pieces.append((int(fr[0]), bits)); lo += n
    assert lo == x.size
    if b.kind == "nemo":
        fr, bits = b.host_io([0], None, PCM_F32, out)
        pieces.append((int(fr[0]), bits))
    if b.kind == "kaldi":
        got = np.concatenate([to_f64(bits, out).reshape(k, b.nm) for k, bits in pieces], axis=0)
    else:
        got = np.concatenate([to_f64(bits, out).reshape(b.nm, k) for k, bits in pieces], axis=1)
    assert got.shape == want.shape, (got.shape, want.shape)
    d = np.abs(got - want)
    d[np.isnan(d)] = np.inf
    print(f"\nSTREAM-BANKS-IO-ORACLE {name} out={out}: worst {d.max():.3e}, gate {gate:.3e} + half ulp <= {half_ulp(want, out).max():.3e}")
    assert (d - (gate + half_ulp(want, out))).max() <= 0.0, float(d.max())


# ---- 9. (pcm, OUT_F32) through the _io calls ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kaldi_40", "nemo_80_f32", "nemo_128_nocenter_f64"])
def test_f32_rows_through_io_are_the_existing_call(gpu, banks, twins, name):
    """(F32, F32) and (S16, F32) through the _io calls, host and device form: the bits of the existing calls, rows and stats.  (The bank
    shows no way to see its typed scratch from outside: only the bits are asserted.)"""
    s16, f32, pushes, want, want_stats = twins(name)
    b = banks(name)
    fence = fence_for(gpu)
    for pcm in (PCM_F32, PCM_S16):
        assert b.bank.supports_io(pcm, OUT_F32)
        src = s16 if pcm == PCM_S16 else f32
        for form in ("host", "device"):
            b.fresh()
            call = (lambda k, ids, ch: b.host_io(ids, ch, pcm, OUT_F32)) if form == "host" else (lambda k, ids, ch: b.dev_io(fence, ids, ch, pcm, OUT_F32))
            same_pushes(drive(b, src, pushes, call), want, OUT_F32, f"{name} {form} ({pcm}, F32)")
            same_stats(b, want_stats, f"{name} {form} ({pcm}, F32)")
    assert not b.bank.supports_io(PCM_F32, 9) and not b.bank.supports_io(7, OUT_F16)
    fence.buf.free()


# ---- CPU ---------------------------------------------------------------------------------------------------------------------------

def test_symbols_everywhere():
    from mel_spec_amd import _lib
    L = _lib.lib()
    rs = open(os.path.join(ROOT, "mel_spec_amd", "rust", "hip.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "melspec_hip.hpp")).read()
    hdr = open(os.path.join(ROOT, "include", "melspec_hip.h")).read()
    for s in SYMBOLS:
        assert hasattr(L, s) and s in _lib.SIGNATURES, s
        assert re.search(r"\b%s\s*\(" % s, hdr), f"{s} is not declared in melspec_hip.h"
        assert re.search(r"fn\s+%s\s*\(" % s, rs), f"{s} is not bound in hip.rs"
        assert re.search(r"\b%s\s*\(" % s, hpp), f"{s} is not used by melspec_hip.hpp"
    assert L.melspec_abi_version() == 1
    import mel_spec_amd as M
    for cls, methods in ((M.FbankStreamBank, ("supports_io", "push_io", "push_device_io")),
                         (M.BlmStreamBank, ("supports_io", "push_io", "finish_io", "push_device_io", "finish_device_io"))):
        for m in methods:
            assert callable(getattr(cls, m)), (cls.__name__, m)


def test_null_bank_needs_no_device():
    """every new entry point with a NULL bank: MELSPEC_ERR_INVALID_ARG with "NULL" in melspec_last_error (supports_io: 0), for every pair of
    codes, known or not -- the handle is looked at first"""
    from mel_spec_amd import _lib
    L = _lib.lib()
    u32 = (C.c_uint32 * 2)(0, 1)
    buf = (C.c_float * 8)()
    p = C.cast(buf, C.c_void_p)
    for pcm, out in [(PCM_F32, OUT_F32), (PCM_S16, OUT_F32)] + TYPED + [(7, OUT_F16), (PCM_S16, 9)]:
        assert L.melspec_fbank_stream_supports_io(None, pcm, out) == 0 and L.melspec_blm_stream_supports_io(None, pcm, out) == 0
        calls = [
            lambda: L.melspec_fbank_stream_push_host_io(None, u32, p, pcm, u32, 1, p, out, 8, u32),
            lambda: L.melspec_fbank_stream_push_device_io(None, u32, p, pcm, None, u32, 1, p, out, None, u32, None),
            lambda: L.melspec_fbank_stream_push_device_io(None, u32, None, pcm, None, u32, 1, p, out, None, u32, None),
            lambda: L.melspec_blm_stream_push_host_io(None, u32, p, pcm, u32, 1, p, out, 8, u32),
            lambda: L.melspec_blm_stream_push_device_io(None, u32, p, pcm, None, u32, 1, p, out, None, u32, None),
            lambda: L.melspec_blm_stream_push_device_io(None, u32, None, pcm, None, u32, 1, p, out, None, u32, None),
            lambda: L.melspec_blm_stream_finish_host_io(None, u32, 1, p, out, 8, u32),
            lambda: L.melspec_blm_stream_finish_device_io(None, u32, 1, p, out, None, u32, None),
        ]
        for k, call in enumerate(calls):
            assert call() == ERR_INVALID_ARG, (k, pcm, out)
            assert "NULL" in _lib.last_error(), (k, pcm, out, _lib.last_error())
