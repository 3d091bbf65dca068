"""NeMo / Parakeet frontend: ragged batches whose clip table lives in device memory (melspec_blm_compute_ragged_device_desc) -- offsets,
lengths and output offsets are read by a planner kernel, nothing is copied back, and two bounds of the caller's hold the table to what the
launch was sized for.

The yardstick everywhere is the EXISTING host-table call, melspec_blm_compute_ragged_device, on the same tables: every output is compared
bit for bit, whole allocation against whole allocation -- both calls write into a fenced buffer filled with a NaN-payload sentinel no
kernel computes (tests/test_io_dtypes.py: Fence), so an element between or behind the clips' rows that one call touches and the other
does not is a difference too; the helper also checks by itself that every such element is still the sentinel.  What is checked:
  1. the edge batch of tests/test_blm_split_ragged.py (1 .. 1001 valid frames and a frameless clip, odd and even sample offsets) in
     every configuration, packed and with the test's own output offsets with gaps, with exact bounds, with slack, with a bound on the
     clip length whose normaliser launch has another shape (480 000 samples) and one whose rows do not fit LDS (8 000 000): the bits do not
     depend on the bounds; the same batch on the kernels of the run-time banks (four waves, six and ten slots); a batch whose own
     longest clip (6.4 minutes) does not fit LDS, where the host-table call runs its one-thread-per-row pass too;
  2. 2500 clips of 0 .. 9 valid frames: several clips per planner thread, threads without a clip;
  3. rejection: a clip longer than max_clip_samples, a batch one column past max_total_columns, d_rejected;
  4. ordering: two calls back to back on one stream without a synchronise, then the context's stream and a caller's;
  5. refusals; 6. the Python entry point.
CPU: the symbol everywhere, the C99 header, the NULL context, and the host half (tests/cpp/blm_desc_plan_host.cpp), plain and sanitized."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_blm_split import VALID_FRAMES, frontend
from test_blm_split_ragged import flatten, samples_for
from test_io_dtypes import ERR_INVALID_ARG, ERR_UNSUPPORTED, OUT_F32, Fence, _upload

SYMBOLS = ["melspec_blm_supports_desc", "melspec_blm_compute_ragged_device_desc"]
REJECTED_UNTOUCHED = 0xFFFFFFFF


def _tab(gpu, a):
    return _upload(gpu, np.ascontiguousarray(a, dtype=np.uint64))


def layout(fe, lens, out_offs):
    """-> (first float of each clip's rows, floats per clip, floats the output spans): packed in clip order, or the test's own offsets"""
    nm = fe.config.n_mels
    sizes = [nm * fe.padded_frames(int(n)) for n in lens]
    if out_offs is None:
        at = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        return at, sizes, int(sum(sizes))
    at = np.asarray(out_offs, np.int64)
    return at, sizes, int(max(a + s for a, s in zip(at, sizes)))


def check_owned(bits, sentinel, at, sizes, what):
    owned = np.zeros(bits.size, bool)
    for a, size in zip(at, sizes):
        assert not owned[a:a + size].any(), "the test's own offsets overlap"
        owned[a:a + size] = True
    left = (bits == sentinel) & owned
    assert not left.any(), f"{what}: {int(left.sum())} elements of the clips' rows never written (first at {int(np.argmax(left))})"
    stray = (bits != sentinel) & ~owned
    assert not stray.any(), f"{what}: {int(stray.sum())} elements between or behind the clips' rows were written (first at {int(np.argmax(stray))})"


def run_host(gpu, fe, d_pcm, offs, lens, out_offs, span):
    """the yardstick: melspec_blm_compute_ragged_device into a fenced output of `span` floats -> its bits"""
    f = Fence(gpu, max(span, 1), OUT_F32)
    fe.compute_ragged_device(d_pcm, offs, lens, f.ptr, out_offs)
    fe.synchronize()
    return f.bits(), f.s


class Desc:
    """one _desc call's device side: the three tables, a fenced output, the u32 for the rejected count (preset to 0xFFFFFFFF)"""

    def __init__(self, gpu, offs, lens, out_offs, span):
        self.gpu, self.n = gpu, len(lens)
        self.t_off, self.t_len = _tab(gpu, offs), _tab(gpu, lens)
        self.t_out = None if out_offs is None else _tab(gpu, out_offs)
        self.fence = Fence(gpu, max(span, 1), OUT_F32)
        self.rej = _upload(gpu, np.array([REJECTED_UNTOUCHED] * 4, np.uint32))

    def call(self, fe, d_pcm, max_cols, max_len, stream=0, n_clips=None, null=()):
        vp = lambda name, p: None if name in null or not p else C.c_void_p(p)
        return self.gpu._lib.lib().melspec_blm_compute_ragged_device_desc(
            fe._h, vp("pcm", d_pcm), vp("offs", self.t_off.ptr), vp("lens", self.t_len.ptr), self.n if n_clips is None else n_clips, vp("out", self.fence.ptr),
            vp("out_offs", self.t_out.ptr if self.t_out else 0), max_cols, max_len, vp("rejected", self.rej.ptr), vp("stream", stream))

    def result(self):
        """after a synchronise -> (bits, rejected); frees everything"""
        bits = self.fence.bits()
        rejected = int(self.rej.download(4, np.uint32)[0])
        for b in (self.t_off, self.t_len, self.t_out, self.rej):
            if b is not None:
                b.free()
        return bits, rejected


def run_desc(gpu, fe, d_pcm, offs, lens, out_offs, span, max_cols, max_len):
    d = Desc(gpu, offs, lens, out_offs, span)
    rc = d.call(fe, d_pcm, max_cols, max_len)
    fe.synchronize()
    bits, rejected = d.result()
    assert rc == 0, gpu._lib.lib().melspec_last_error()
    return bits, rejected


def assert_same_bits(got, want, what):
    diff = got != want
    assert not diff.any(), f"{what}: {int(diff.sum())} elements differ from melspec_blm_compute_ragged_device on the same tables (first at {int(np.argmax(diff))})"


def gapped_offsets(fe, lens):
    """the clips' rows in reverse clip order with gaps of 1, 3 and 64 floats in front of them"""
    offs, cur = [0] * len(lens), 0
    for k, c in enumerate(reversed(range(len(lens)))):
        cur += (1, 3, 64)[k % 3]
        offs[c] = cur
        cur += fe.config.n_mels * fe.padded_frames(int(lens[c]))
    return offs, cur + 3


# ---- Test 1: the edge batch ---------------------------------------------------------------------------------------------------------------

_CLIPS = {}


def edge_clips(oracle, center):
    if center not in _CLIPS:
        order = np.random.default_rng(4).permutation(len(VALID_FRAMES))
        valid = [VALID_FRAMES[i] for i in order]
        clips = [oracle.synth_pcm(300 + v, samples_for(v, center)) for v in valid]
        valid.insert(6, 0)          # in the middle: a clip without a frame -- center = 0: 300 samples (fewer than n_fft); centred: no sample at all
        clips.insert(6, oracle.synth_pcm(7, 0 if center else 300))
        _CLIPS[center] = (clips, valid)
    return _CLIPS[center]


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [0, 1], ids=["raw", "normalised"])
@pytest.mark.parametrize("pad_to", [0, 16])
@pytest.mark.parametrize("center", [True, False], ids=["center", "nocenter"])
@pytest.mark.parametrize("mode", ["f64", "f32"])
@pytest.mark.parametrize("nm", [80, 128])
def test_edge_batch_is_the_host_table_calls_bits(gpu, oracle, nm, mode, center, pad_to, norm):
    clips, valid = edge_clips(oracle, center)
    fe = frontend(gpu, nm, mode, pad_to=pad_to, center=center, preemphasis=0.97, normalize_per_feature=bool(norm))
    assert gpu._lib.lib().melspec_blm_supports_desc(fe._h) == 1
    flat, offs, lens = flatten(clips)
    assert {int(o) & 1 for o in offs} == {0, 1}, "odd and even sample offsets"
    assert [fe.num_frames(int(n)) for n in lens] == valid
    total, longest = sum(fe.padded_frames(int(n)) for n in lens), int(lens.max())
    d = _upload(gpu, flat)
    for out_offs, span in ((None, None), gapped_offsets(fe, lens)):
        at, sizes, packed_span = layout(fe, lens, out_offs)
        span = packed_span if span is None else span
        want, sentinel = run_host(gpu, fe, d.ptr, offs, lens, out_offs, span)
        check_owned(want, sentinel, at, sizes, "the yardstick")
        for max_cols, max_len in ((total, longest), (total + 1234, longest * 10), (total, 480000), (total + 1, 8000000)):
            what = f"{nm} {mode} center {center} pad_to {pad_to} norm {norm} {'packed' if out_offs is None else 'offsets'} bounds ({max_cols}, {max_len})"
            got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, out_offs, span, max_cols, max_len)
            check_owned(got, sentinel, at, sizes, what)
            assert_same_bits(got, want, what)
            assert rejected == 0, what
    d.free()
    fe.close()


@pytest.mark.gpu
@pytest.mark.parametrize("nm", [3, 5, 40, 140])
def test_edge_batch_on_the_run_time_banks(gpu, oracle, nm):
    """the other kernels a batch of this frontend can run on (fused512_route.hpp): four f64 waves (3 mels), eight with run-time slot lengths,
    six slots (5, 40 mels) and ten (140) -- each reads the true unit count from the plan like the compile-time banks' kernels"""
    clips, valid = edge_clips(oracle, True)
    fe = frontend(gpu, nm, "f64", pad_to=16, preemphasis=0.97, normalize_per_feature=True)
    assert gpu._lib.lib().melspec_blm_supports_desc(fe._h) == 1
    flat, offs, lens = flatten(clips)
    total, longest = sum(fe.padded_frames(int(n)) for n in lens), int(lens.max())
    d = _upload(gpu, flat)
    out_offs, span = gapped_offsets(fe, lens)
    at, sizes, _ = layout(fe, lens, out_offs)
    want, sentinel = run_host(gpu, fe, d.ptr, offs, lens, out_offs, span)
    for max_cols, max_len in ((total, longest), (total + 1234, longest * 10)):
        got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, out_offs, span, max_cols, max_len)
        check_owned(got, sentinel, at, sizes, f"{nm} mels bounds ({max_cols}, {max_len})")
        assert_same_bits(got, want, f"{nm} mels bounds ({max_cols}, {max_len})")
        assert rejected == 0
    d.free()
    fe.close()


@pytest.mark.gpu
def test_a_clip_whose_rows_do_not_fit_lds(gpu):
    """38 126 valid frames: the host-table call's normaliser is the one-thread-per-row pass (a left fold, a division per element), and so
    is this call's -- for the long clip and for the short ones beside it"""
    lens = np.array([16007, 6100000, 0, 4800], np.uint64)
    offs = np.array([1, 16010, 6116011, 6116012], np.uint64)
    flat = (np.random.default_rng(61).standard_normal(int(offs[-1] + lens[-1]) + 1) * 0.1).astype(np.float32)
    fe = frontend(gpu, 80, "f64", normalize_per_feature=True, preemphasis=0.97)
    total, longest = sum(fe.padded_frames(int(n)) for n in lens), int(lens.max())
    assert fe.num_frames(longest) == 38126
    at, sizes, span = layout(fe, lens, None)
    d = _upload(gpu, flat)
    want, sentinel = run_host(gpu, fe, d.ptr, offs, lens, None, span)
    for max_cols, max_len in ((total, longest), (total + 1234, longest * 10)):
        got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, None, span, max_cols, max_len)
        check_owned(got, sentinel, at, sizes, f"bounds ({max_cols}, {max_len})")
        assert_same_bits(got, want, f"bounds ({max_cols}, {max_len})")
        assert rejected == 0
    d.free()
    fe.close()


# ---- Test 2: many tiny clips --------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_many_tiny_clips(gpu, mode):
    """2500 clips of 0 .. 9 valid frames: three clips per planner thread, 190 threads without one; normalised, 80 mels"""
    rng = np.random.default_rng(25)
    valid = rng.integers(0, 10, 2500)
    lens = np.where(valid == 0, 0, (valid - 1) * 160 + rng.integers(1, 160, 2500)).astype(np.uint64)
    gaps = rng.integers(0, 3, 2500)
    offs = (np.cumsum(np.concatenate([[1], lens[:-1].astype(np.int64) + gaps[:-1]]))).astype(np.uint64)
    flat = (np.random.default_rng(26).standard_normal(int(offs[-1] + lens[-1]) + 1) * 0.1).astype(np.float32)
    fe = frontend(gpu, 80, mode, normalize_per_feature=True, preemphasis=0.97)
    assert [fe.num_frames(int(n)) for n in lens[:50]] == list(valid[:50])
    total, longest = sum(fe.padded_frames(int(n)) for n in lens), int(lens.max())
    at, sizes, span = layout(fe, lens, None)
    d = _upload(gpu, flat)
    want, sentinel = run_host(gpu, fe, d.ptr, offs, lens, None, span)
    for max_cols, max_len in ((total, longest), (total + 1234, longest * 10)):
        got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, None, span, max_cols, max_len)
        check_owned(got, sentinel, at, sizes, f"{mode} bounds ({max_cols}, {max_len})")
        assert_same_bits(got, want, f"{mode} bounds ({max_cols}, {max_len})")
        assert rejected == 0
    d.free()
    fe.close()


# ---- Test 3: rejection --------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("own_offsets", [False, True], ids=["packed", "offsets"])
@pytest.mark.parametrize("nm,mode", [(80, "f64"), (128, "f32")])
def test_rejection_is_decided_on_the_device(gpu, oracle, nm, mode, own_offsets):
    """The output allocation holds the WHOLE batch, the rejected clip's rows included: a planner that ignored a bound fails an assertion
    here, not the device."""
    lens_in = [4000, 16007, 1, 48000, 0, 2400, 9999]
    clips = [oracle.synth_pcm(40 + c, n) for c, n in enumerate(lens_in)]
    flat, offs, lens = flatten(clips)
    fe = frontend(gpu, nm, mode, pad_to=16, preemphasis=0.97, normalize_per_feature=False)
    d = _upload(gpu, flat)
    total = sum(fe.padded_frames(int(n)) for n in lens)
    out_offs, span = gapped_offsets(fe, lens) if own_offsets else (None, layout(fe, lens, None)[2])
    # (A) the 3 s clip in the middle is longer than the bound: the others equal the yardstick on the table with that length set to 0
    cut = lens.copy()
    cut[3] = 0
    want, sentinel = run_host(gpu, fe, d.ptr, offs, cut, out_offs, span)
    at, sizes, _ = layout(fe, cut, out_offs)
    check_owned(want, sentinel, at, sizes, "the yardstick")
    for max_cols in (total, total - fe.padded_frames(48000)):           # room for the whole table; room for exactly what survives (A)
        got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, out_offs, span, max_cols, 16007)
        check_owned(got, sentinel, at, sizes, "(A)")                   # the rejected clip's rows (own offsets: where the table puts them) stay sentinel
        assert_same_bits(got, want, f"(A), max_total_columns {max_cols}")
        assert rejected == 1
    # (B) one column short of the true total: nothing is written, every clip is rejected
    got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, out_offs, span, total - 1, 48000)
    assert np.all(got == sentinel), f"(B): {int((got != sentinel).sum())} elements written"
    assert rejected == len(lens)
    # ... also when (A) has rejected a clip first and the survivors are one column over
    got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, out_offs, span, total - fe.padded_frames(48000) - 1, 16007)
    assert np.all(got == sentinel) and rejected == len(lens)
    # exact bounds: nobody is rejected
    want, _ = run_host(gpu, fe, d.ptr, offs, lens, out_offs, span)
    got, rejected = run_desc(gpu, fe, d.ptr, offs, lens, out_offs, span, total, 48000)
    assert_same_bits(got, want, "exact bounds")
    assert rejected == 0
    d.free()
    fe.close()


# ---- Test 4: ordering ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("norm", [0, 1], ids=["raw", "normalised"])
def test_calls_back_to_back_and_on_two_streams(gpu, oracle, norm):
    """Two calls with different tables on one stream with nothing between them: the second planner overwrites the plan the first launch read,
    in stream order.  Then a call on the context's stream and one on a caller's stream."""
    fe = frontend(gpu, 80, "f64", normalize_per_feature=bool(norm), preemphasis=0.97)
    batches = []
    for seed, lens_in in ((60, [16007, 0, 320, 4800, 33, 160000, 5120]), (70, [9999, 48000, 1, 2400])):
        flat, offs, lens = flatten([oracle.synth_pcm(seed + c, n) for c, n in enumerate(lens_in)])
        d = _upload(gpu, flat)
        at, sizes, span = layout(fe, lens, None)
        want, _ = run_host(gpu, fe, d.ptr, offs, lens, None, span)
        batches.append((d, offs, lens, span, want, sum(fe.padded_frames(int(n)) for n in lens), int(lens.max())))
    for streams in ((None, None), (None, torch.cuda.Stream()), (torch.cuda.Stream(), None)):          # None: the context's own stream
        calls = []
        for (d, offs, lens, span, want, total, longest), st in zip(batches, streams):
            k = Desc(gpu, offs, lens, None, span)
            assert k.call(fe, d.ptr, total + 100, longest + 7, stream=0 if st is None else st.cuda_stream) == 0, gpu._lib.lib().melspec_last_error()
            calls.append(k)
        for st in streams:
            fe.synchronize() if st is None else st.synchronize()
        for k, b in zip(calls, batches):
            got, rejected = k.result()
            assert_same_bits(got, b[4], f"caller streams {[s is not None for s in streams]}")
            assert rejected == 0
    for b in batches:
        b[0].free()
    fe.close()


# ---- Test 5: refusals ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_refusals_write_nothing(gpu, oracle):
    last = lambda: gpu._lib.lib().melspec_last_error().decode()
    flat, offs, lens = flatten([oracle.synth_pcm(c, n) for c, n in enumerate((4000, 1234))])
    d = _upload(gpu, flat)

    def refused(fe, max_cols=1000, max_len=4000, **kw):
        k = Desc(gpu, offs, lens, None, 128 * 1000)
        rc = k.call(fe, d.ptr, max_cols, max_len, **kw)
        fe.synchronize()
        bits, rejected = k.result()
        assert np.all(bits == k.fence.s), f"a call that computes nothing wrote {int((bits != k.fence.s).sum())} elements"
        assert rejected == REJECTED_UNTOUCHED, "a call that queues nothing wrote d_rejected"
        return rc

    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(n_fft=400, win_length=400))           # the generic kernel
    assert gpu._lib.lib().melspec_blm_supports_desc(fe._h) == 0
    assert refused(fe) == ERR_UNSUPPORTED
    assert "fused kernel" in last()
    assert refused(fe, n_clips=0, null=("pcm", "offs", "lens", "out")) == ERR_UNSUPPORTED      # before everything but the NULL context
    fe.close()
    fe = frontend(gpu, 80, "f64", normalize_per_feature=True)
    assert refused(fe, n_clips=0) == 0
    assert refused(fe, max_cols=0) == 0 and refused(fe, max_len=0) == 0
    assert refused(fe, n_clips=0, null=("pcm", "offs", "lens", "out")) == 0                     # ... and before the pointers
    for ptr in ("pcm", "out", "offs", "lens"):
        assert refused(fe, null=(ptr,)) == ERR_INVALID_ARG, ptr
        assert "NULL" in last()
    assert refused(fe, max_cols=1 << 40) == ERR_UNSUPPORTED and "device plan" in last()
    assert refused(fe, max_len=160 << 31) == ERR_UNSUPPORTED
    # NULL d_rejected and NULL output offsets are fine
    k = Desc(gpu, offs, lens, None, 80 * 40)
    assert k.call(fe, d.ptr, 40, 4000, null=("rejected",)) == 0
    fe.synchronize()
    bits, rejected = k.result()
    assert rejected == REJECTED_UNTOUCHED and not np.any(bits[:80 * (fe.padded_frames(4000) + fe.padded_frames(1234))] == k.fence.s)
    d.free()
    fe.close()


# ---- Test 6: the Python entry point -------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("norm", [False, True], ids=["raw", "normalised"])
def test_python_function_on_jfk_in_five_pieces(gpu, jfk, norm):
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(preemphasis=0.97, normalize_per_feature=norm))
    cuts = [0, 30001, 30001 + 16000, 90000, 130007, len(jfk)]
    offs = np.array(cuts[:-1], np.uint64)
    lens = np.array([b - a for a, b in zip(cuts[:-1], cuts[1:])], np.uint64)
    at, sizes, span = layout(fe, lens, None)
    d = _upload(gpu, jfk)
    want, sentinel = run_host(gpu, fe, d.ptr, offs, lens, None, span)
    t_off, t_len, rej, out = _tab(gpu, offs), _tab(gpu, lens), _upload(gpu, np.zeros(4, np.uint32) + 9), Fence(gpu, span, OUT_F32)
    gpu.blm_compute_ragged_device_desc(fe, d.ptr, t_off.ptr, t_len.ptr, len(lens), out.ptr, 0, span // fe.config.n_mels, int(lens.max()), rej.ptr)
    fe.synchronize()
    got = out.bits()
    check_owned(got, sentinel, at, sizes, "jfk")
    assert_same_bits(got, want, "jfk in five pieces")
    assert int(rej.download(4, np.uint32)[0]) == 0
    for b in (d, t_off, t_len, rej):
        b.free()
    fe.close()


# ---- CPU ----------------------------------------------------------------------------------------------------------------------------------

def test_desc_symbols_everywhere():
    """the entry points resolve in the built library and are declared in the header, the ctypes table, the C++ wrapper and the Rust shim; the
    ABI version is still 1 and the header is still C99"""
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
        assert re.search(rf"\b{sym}\s*\(", header)
        assert f'"{sym}"' in table
        assert re.search(rf"\b{sym}\s*\(", wrapper)
        assert re.search(rf"\bfn {sym}\s*\(", shim)
    assert re.search(r"\bunsafe fn compute_ragged_device_desc\s*\(&mut self, d_pcm", shim)
    assert callable(mel_spec_amd.blm_compute_ragged_device_desc) and "blm_compute_ragged_device_desc" in mel_spec_amd.__all__
    assert not hasattr(mel_spec_amd.BatchLogMelSpectrogram, "compute_ragged_device_desc")       # a function: the classes' attributes are a pinned set
    assert lib.melspec_abi_version() == 1
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-x", "c", header_path])


def test_desc_null_context_needs_no_device():
    from mel_spec_amd import _lib
    lib = _lib.lib()
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.melspec_blm_compute_ragged_device_desc(None, p, p, p, 1, p, None, 100, 1000, p, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_compute_ragged_device_desc(None, None, None, None, 0, None, None, 0, 0, None, None) == ERR_INVALID_ARG
    assert b"blm is NULL" in lib.melspec_last_error()
    assert lib.melspec_blm_supports_desc(None) == 0
    assert np.all(buf == 0)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_desc_plan_on_the_host(tmp_path, sanitize):
    """the arithmetic the planner kernel shares with the host (mel_spec_amd/csrc/blm_desc_plan.hpp: frame counts, the plan buffer's layout,
    rules (A) and (B), the serial planner, the normaliser's launch shape) as a stand-alone program, plain and with
    -fsanitize=address,undefined: tests/cpp/blm_desc_plan_host.cpp"""
    exe = tmp_path / "blm_desc_plan_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "blm_desc_plan_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.startswith("blm_desc_plan_host: ok"), p.stdout + p.stderr
