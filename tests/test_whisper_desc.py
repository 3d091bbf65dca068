"""The centred Whisper features from a clip table in device memory (melspec_whisper_compute_ragged_device_desc*) on the GPU.

Yardstick 1, everywhere: the EXISTING host-table call on the same tables, np.array_equal over the whole output -- both calls write into an
allocation filled with the NaN-payload sentinel of its type between two guard bands (tests/test_whisper_centered_io.py: Fence), so an
element between or behind the clips' outputs that one call touches and the other does not is a difference too; check_owned asserts by
itself that every element of a clip's output was written and no other.  Yardstick 2, where named: tests/whisper_centered_ref.py at the
gates of tests/test_whisper_centered.py (F64_TOL 2e-6, F32_TOL 6e-4, raw rows at 4 x F64_TOL in f64 only, the returned maximum bit for
bit the f32 maximum of the returned rows), on inputs the host-table call already passes at those gates.

The samples between the clips of an input buffer are loud (1e3, int16 32767): a frame that read one would be heard in the bits."""
import ctypes as C

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py); a caller's stream and the device-side table copies come from here

import mel_spec_amd as M
import whisper_centered_ref as R
from test_io_dtypes import ERR_INVALID_ARG, ERR_UNSUPPORTED, OUT_BF16, OUT_F16, OUT_F32, PCM_F32, PCM_S16, to_f32
from test_whisper_centered import DEVICE_PADS, F32_TOL, F64_TOL, MODE_IDS, MODES, PADDED, TILE_PAD_N, TILE_PADS, _pad_lengths, make, noise, ref, worst
from test_whisper_centered_io import Fence, s16_clips

pytestmark = pytest.mark.gpu


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
def dev(a, dtype=None):
    from mel_spec_amd.hip import DeviceBuffer
    a = np.ascontiguousarray(a, dtype)
    d = DeviceBuffer(max(a.nbytes, 16))
    if a.nbytes:
        d.upload(a)
    return d


def lay_out(clips, dtype, gaps):
    """the clips in one host array of `dtype`, gaps[i] loud samples in front of clip i and three behind the last; the first clip starts at gaps[0]"""
    loud = 32767 if dtype == np.int16 else 1e3
    offs, cur = [], 0
    for g, c in zip(gaps, clips):
        cur += int(g)
        offs.append(cur)
        cur += c.shape[0]
    flat = np.full(cur + 3, loud, dtype)
    for o, c in zip(offs, clips):
        flat[o:o + c.shape[0]] = c
    return flat, np.array(offs, np.uint64), np.array([c.shape[0] for c in clips], np.uint64)


def check_owned(bits, sentinel, at, sizes, what):
    owned = np.zeros(bits.size, bool)
    for a, size in zip(at, sizes):
        assert not owned[a:a + size].any(), "the test's own offsets overlap"
        owned[a:a + size] = True
    left = (bits == sentinel) & owned
    assert not left.any(), f"{what}: {int(left.sum())} elements of the clips' outputs never written (first at {int(np.argmax(left))})"
    stray = (bits != sentinel) & ~owned
    assert not stray.any(), f"{what}: {int(stray.sum())} elements between or behind the clips' outputs were written (first at {int(np.argmax(stray))})"


def assert_same_bits(got, want, what):
    assert got.shape == want.shape
    diff = got != want
    assert not diff.any(), f"{what}: {int(diff.sum())} elements differ from the host-table call on the same tables (first at {int(np.argmax(diff))})"


class Call:
    """one call queued on `stream` (not waited for): a fenced output of `span + shift` elements and, for a split call, fenced maxima.
    desc: the tables are device arrays (tabs = (d_off, d_len, d_dst_off or 0) device pointers, or None: uploaded here); otherwise the
    host-table call on offs / lens / dst_offs."""

    def __init__(self, mel, desc, d_pcm, offs, lens, pad_to, split=False, mel_major=True, pcm=PCM_F32, out=OUT_F32, dst_offs=None, span=None, shift=0, stream=0,
                 tabs=None, launch=True):
        """launch = False: everything is allocated and uploaded here, launch() queues the call -- nothing of the test's stands between two launches"""
        n, T = len(lens), pad_to // 160
        self.span = n * T * mel.n_mels if span is None else span
        self.shift, self.f, self.mx = shift, Fence(self.span + shift, out), Fence(n, OUT_F32) if split else None
        self.own = []
        ptr, io = self.f.ptr + shift * self.f.es, (pcm, out) != (PCM_F32, OUT_F32)
        oo = None if dst_offs is None else [int(o) for o in dst_offs]
        if desc:
            if tabs is None:
                self.own = [dev(offs, np.uint64), dev(lens, np.uint64)] + ([dev(oo, np.uint64)] if oo is not None else [])
                tabs = (self.own[0].ptr, self.own[1].ptr, self.own[2].ptr if oo is not None else 0)
        self.launch = lambda: self._launch(mel, desc, d_pcm, offs, lens, n, pad_to, split, mel_major, pcm, out, io, oo, ptr, stream, tabs)
        if launch:
            self.launch()

    def _launch(self, mel, desc, d_pcm, offs, lens, n, pad_to, split, mel_major, pcm, out, io, oo, ptr, stream, tabs):
        if desc:
            if split and io:
                M.whisper_ragged_device_desc_split_io(mel, d_pcm, pcm, tabs[0], tabs[1], n, ptr, out, self.mx.ptr, pad_to, tabs[2], stream)
            elif split:
                M.whisper_ragged_device_desc_split(mel, d_pcm, tabs[0], tabs[1], n, ptr, self.mx.ptr, pad_to, tabs[2], stream)
            elif io:
                M.whisper_ragged_device_desc_io(mel, d_pcm, pcm, tabs[0], tabs[1], n, ptr, out, pad_to, tabs[2], mel_major, stream)
            else:
                M.whisper_ragged_device_desc(mel, d_pcm, tabs[0], tabs[1], n, ptr, pad_to, tabs[2], mel_major, stream)
        elif split and io:
            M.whisper_ragged_device_split_io(mel, d_pcm, pcm, offs, lens, ptr, out, self.mx.ptr, pad_to, oo, stream)
        elif split:
            M.whisper_ragged_device_split(mel, d_pcm, offs, lens, ptr, self.mx.ptr, pad_to, oo, stream)
        elif io:
            M.whisper_ragged_device_io(mel, d_pcm, pcm, offs, lens, ptr, out, pad_to, oo, mel_major, stream)
        else:
            M.whisper_ragged_device(mel, d_pcm, offs, lens, ptr, pad_to, oo, mel_major, stream)

    def result(self):
        """after a synchronise -> (the output's bits past the shift, the maxima's bits or None, the sentinel); frees everything"""
        bits = self.f.bits()
        assert np.all(bits[:self.shift] == self.f.s), "an element in front of the shifted pointer was written"
        g = self.mx.bits().copy() if self.mx else None
        for b in [self.f, self.mx] + self.own:
            if b is not None:
                b.free()
        return bits[self.shift:].copy(), g, self.f.s


def both(mel, d_pcm, offs, lens, pad_to, what, **kw):
    """the host-table call and the _desc call on the same tables, each waited for: yardstick 1 and check_owned -> (bits, maxima bits)"""
    n, T, nm = len(lens), pad_to // 160, mel.n_mels
    at = [i * T * nm for i in range(n)] if kw.get("dst_offs") is None else [int(o) for o in kw["dst_offs"]]
    res = []
    for desc in (False, True):
        c = Call(mel, desc, d_pcm, offs, lens, pad_to, **kw)
        mel.synchronize(kw.get("stream", 0))
        res.append(c.result())
    (want, g_w, s), (got, g, _) = res
    check_owned(want, s, at, [T * nm] * n, what + ": the yardstick")
    check_owned(got, s, at, [T * nm] * n, what)
    assert_same_bits(got, want, what)
    if g is not None:
        assert np.array_equal(g, g_w), f"{what}: d_clip_max differs from the host-table call's"
    return got, g


def as_f32(bits):
    return bits.view(np.float32)


def against_ref(mel, key, clips, pad_to, tol, raw_direct, d_pcm, offs, lens, what):
    """normalised mel-major and frame-major and split through the _desc calls: yardstick 1 for each (both), then yardstick 2"""
    n, T, nm = len(lens), pad_to // 160, mel.n_mels
    mm, _ = both(mel, d_pcm, offs, lens, pad_to, what + " mel-major", mel_major=True)
    fm, _ = both(mel, d_pcm, offs, lens, pad_to, what + " frame-major", mel_major=False)
    rows, g = both(mel, d_pcm, offs, lens, pad_to, what + " split", split=True)
    mm, fm, rows, g = as_f32(mm).reshape(n, nm, T), as_f32(fm).reshape(n, T, nm), as_f32(rows).reshape(n, T, nm), as_f32(g)
    w_n = w_r = w_g = 0.0
    for i, (raw, gw, nrm) in enumerate(ref(key, clips, pad_to, nm)):
        assert np.array_equal(mm[i].T, fm[i]), f"{what}: clip {i}: mel-major and frame-major bits differ"
        w_n = max(w_n, worst(fm[i], nrm))
        w_g = max(w_g, abs(float(g[i]) - gw))
        assert g[i] == np.float32(rows[i].max()), f"{what}: clip {i}: maximum {g[i]!r}, the largest returned value {rows[i].max()!r}"
        w_r = max(w_r, worst(rows[i], raw) if raw_direct else worst(R.fold_f32(rows[i], g[i]), nrm))
    print(f"{what}: normalised {w_n:.3e} (gate {tol:.0e}), g {w_g:.3e}, split {'raw' if raw_direct else 'folded'} {w_r:.3e}")
    assert w_n <= tol, f"{what}: normalised"
    assert w_g <= 4 * tol, f"{what}: clip maxima"
    assert w_r <= (4 * tol if raw_direct else tol), f"{what}: split rows"


# ---- 1. every frame class in one batch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_every_frame_class_in_one_batch(oracle, n_mels, mode, tol):
    clips = [noise(200 + i, n, oracle) for i, n in enumerate(PADDED)]          # test_pad_and_trim's clips: the reference is shared
    flat, offs, lens = lay_out(clips, np.float32, [1 + i % 3 for i in range(len(clips))])
    assert offs[0] == 1
    classes = {R.frame_classes(n, 4800) for n in PADDED}
    # (frames, interior, first_silent): all silent; edges only with a silent tail; an interior with a silent tail; no silent frame at all
    assert (30, 0, 0) in classes and any(i == 0 and 0 < s < 30 for _, i, s in classes) and any(i > 0 and s < 30 for _, i, s in classes) and any(s == 30 for _, _, s in classes)
    mel = make(n_mels, mode)
    assert M.supports_whisper_desc(mel)
    d = dev(flat)
    against_ref(mel, "pad-all", clips, 4800, tol, mode != "f32", d.ptr, offs, lens, f"pad_to 4800 mels {n_mels} mode {mode}")
    d.free(); mel.close()


# ---- 2. other widths ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_other_widths(oracle, n_mels, mode, tol):
    mel = make(n_mels, mode)
    for pad_to in DEVICE_PADS:
        ns = _pad_lengths(pad_to)
        clips = [noise(1200 + i, n, oracle) for i, n in enumerate(ns)]          # test_pad_to_on_the_device's clips
        flat, offs, lens = lay_out(clips, np.float32, [1 + i % 3 for i in range(len(clips))])
        d = dev(flat)
        against_ref(mel, ("device-pad", pad_to), clips, pad_to, tol, mode != "f32", d.ptr, offs, lens, f"pad_to {pad_to} mels {n_mels} mode {mode}")
        d.free()
    mel.close()


# ---- 3. tile boundaries of the finalise pass ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_finalize_tiles(oracle, n_mels, mode, tol):
    clips = [noise(600 + i, n, oracle) for i, n in enumerate(TILE_PAD_N)]         # test_finalize_tiles_at_the_silent_boundary's clips
    mel = make(n_mels, mode)
    for pad_to, T in TILE_PADS.items():
        flat, offs, lens = lay_out(clips, np.float32, [1 + i % 3 for i in range(len(clips))])
        d = dev(flat)
        against_ref(mel, ("tile-pad", pad_to), clips, pad_to, tol, mode != "f32", d.ptr, offs, lens, f"pad_to {pad_to} mels {n_mels} mode {mode}")
        # one element past the 16-byte aligned start: the element-wise store of the mel-major tiles
        both(mel, d.ptr, offs, lens, pad_to, f"pad_to {pad_to}, d_out + 1", mel_major=True, shift=1)
        d.free()
    mel.close()


# ---- 4. the planner's shape ---------------------------------------------------------------------------------------------------------------------
def _many(n, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 2001, n).astype(np.uint64)
    gaps = rng.integers(0, 4, n)
    offs = np.cumsum(np.concatenate([[1], lens[:-1].astype(np.int64) + gaps[:-1]])).astype(np.uint64)
    flat = (rng.standard_normal(int(offs[-1] + lens[-1]) + 3) * 0.1).astype(np.float32)
    return flat, offs, lens


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_2500_clips(mode):
    """three clips per planner thread, 190 threads without one; lengths on both sides of pad_to: every class, trimmed clips, empty clips"""
    flat, offs, lens = _many(2500, 41)
    assert (lens > 1600).any() and (lens < 200).any()
    mel = make(80, mode)
    d = dev(flat)
    both(mel, d.ptr, offs, lens, 1600, f"2500 clips {mode} normalised")
    both(mel, d.ptr, offs, lens, 1600, f"2500 clips {mode} split", split=True)
    d.free(); mel.close()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025])
def test_clip_counts_around_the_planner_width(n):
    """one clip, one short of a clip per planner thread, exactly one each, one thread with two; the suite's mode (test_2500_clips has both)"""
    flat, offs, lens = _many(n, 100 + n)
    mel = make(80)
    d = dev(flat)
    both(mel, d.ptr, offs, lens, 1600, f"{n} clips normalised")
    both(mel, d.ptr, offs, lens, 1600, f"{n} clips split", split=True)
    d.free(); mel.close()


# ---- 5. caller-chosen output offsets in device memory ---------------------------------------------------------------------------------------
def _reversed_with_gaps(n, size):
    offs, cur = [0] * n, 0
    for k, i in enumerate(reversed(range(n))):
        cur += (1, 3, 64, 5)[k % 4]
        offs[i] = cur
        cur += size
    return offs, cur + 3


@pytest.mark.parametrize("n_mels", [80, 128])
def test_output_offsets_from_device_memory(oracle, n_mels):
    ns = [1000, 10040, 0, 5000, 20000, 10239]
    clips = [noise(800 + i, n, oracle) for i, n in enumerate(ns)]
    flat, offs, lens = lay_out(clips, np.float32, [1 + i % 3 for i in range(len(clips))])
    mel = make(n_mels)
    d = dev(flat)
    oo, span = _reversed_with_gaps(len(ns), 64 * n_mels)
    assert {o & 3 for o in oo} != {0}, "the offsets turn the 16-byte path off for some clips"
    for kw in ({"mel_major": True}, {"mel_major": False}, {"split": True}):
        packed, g_p = both(mel, d.ptr, offs, lens, 10240, f"packed {kw}", **kw)
        got, g = both(mel, d.ptr, offs, lens, 10240, f"offsets {kw}", dst_offs=oo, span=span, **kw)          # check_owned: every word of every gap keeps its sentinel
        for i, o in enumerate(oo):
            assert np.array_equal(got[o:o + 64 * n_mels], packed[i * 64 * n_mels:(i + 1) * 64 * n_mels]), f"clip {i} at element {o} differs from the packed call"
        if g is not None:
            assert np.array_equal(g, g_p)
    d.free(); mel.close()


# ---- 6. stream order ----------------------------------------------------------------------------------------------------------------------------
def _two_batches(oracle):
    out = []
    for seed, ns in ((60, [4800, 0, 320, 2400, 33, 9000, 4601]), (70, [1, 4799, 700, 200])):
        clips = [noise(seed + i, n, oracle) for i, n in enumerate(ns)]
        out.append(lay_out(clips, np.float32, [1 + i % 3 for i in range(len(clips))]))
    return out


@pytest.mark.parametrize("split", [False, True], ids=["normalised", "split"])
def test_back_to_back_and_on_two_streams(oracle, split):
    """Two calls with different tables on one stream with nothing between them: the second planner overwrites the plan the first call's
    kernels read, in stream order.  Then the same on a caller's stream, and one call on each: with two streams the second call first
    waits for the first call's stream (the plan and scratch buffers are used in stream order, DevicePlan's rule), so those two cases check
    that hand-over, not two calls running at once -- which the context does not promise."""
    mel = make(80)
    batches = []
    for flat, offs, lens in _two_batches(oracle):
        d = dev(flat)
        c = Call(mel, False, d.ptr, offs, lens, 4800, split=split)
        mel.synchronize()
        batches.append((d, offs, lens, c.result()))
    side = torch.cuda.Stream()
    for streams in ((0, 0), (side.cuda_stream, side.cuda_stream), (0, side.cuda_stream), (side.cuda_stream, 0)):
        calls = [Call(mel, True, d.ptr, offs, lens, 4800, split=split, stream=st, launch=False) for (d, offs, lens, _), st in zip(batches, streams)]
        mel.synchronize(); side.synchronize()
        for c in calls:
            c.launch()
        for st in set(streams):
            mel.synchronize(st)
        for c, (_, _, _, (want, g_w, _)) in zip(calls, batches):
            got, g, _ = c.result()
            assert_same_bits(got, want, f"streams {streams}")
            assert g is None or np.array_equal(g, g_w)
    for b in batches:
        b[0].free()
    mel.close()


def test_tables_written_on_the_stream_just_before_the_call(oracle):
    """the tables reach their device arrays by an asynchronous device-side copy on the call's stream, with no host wait in between: the
    planner reads them in stream order.  Before the copy the arrays hold another batch's table."""
    mel = make(80)
    (flat_a, offs_a, lens_a), (flat_b, offs_b, lens_b) = _two_batches(oracle)
    n = len(lens_b)
    flat = np.concatenate([flat_b, flat_a])          # one buffer for both: the stale table's offsets are valid too
    d = dev(flat)
    c = Call(mel, False, d.ptr, offs_b, lens_b, 4800)
    mel.synchronize()
    want, _, _ = c.result()
    side = torch.cuda.Stream()
    src = torch.from_numpy(np.stack([offs_b, lens_b]).astype(np.int64)).cuda()
    stale = np.stack([offs_a[:n] + np.uint64(flat_b.shape[0]), lens_a[:n]]).astype(np.int64)
    torch.cuda.synchronize()
    for st in (torch.cuda.current_stream(), side):
        with torch.cuda.stream(st):
            dst = torch.from_numpy(stale).cuda()
            c = Call(mel, True, d.ptr, None, lens_b, 4800, stream=st.cuda_stream, tabs=(dst[0].data_ptr(), dst[1].data_ptr(), 0), launch=False)
            torch.cuda.synchronize()
            dst.copy_(src, non_blocking=True)          # device to device, on st
            c.launch()
        st.synchronize()
        got, _, _ = c.result()
        assert_same_bits(got, want, "tables copied on the stream in front of the call")
    d.free(); mel.close()


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_same_bits_twice_and_no_stale_scratch(oracle, mode):
    mel = make(80, mode)
    flat, offs, lens = _many(300, 7)                          # a larger batch first: its plan, rows and edge samples stay in the scratch
    d = dev(flat)
    both(mel, d.ptr, offs, lens, 4800, "the larger batch")
    d.free()
    (flat, offs, lens), _ = _two_batches(oracle)
    d = dev(flat)
    for kw in ({}, {"split": True}):
        first, g1 = both(mel, d.ptr, offs, lens, 4800, f"after a larger batch {kw}", **kw)
        again, g2 = both(mel, d.ptr, offs, lens, 4800, f"the same batch again {kw}", **kw)
        assert np.array_equal(first, again) and (g1 is None or np.array_equal(g1, g2))
        fresh = make(80, mode)
        c = Call(fresh, True, d.ptr, offs, lens, 4800, **kw)
        fresh.synchronize()
        got, g3, _ = c.result()
        assert np.array_equal(got, first) and (g1 is None or np.array_equal(g1, g3)), "a used context differs from a fresh one"
        fresh.close()
    d.free(); mel.close()


# ---- 7. 16-bit ends ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pcm,out", [(PCM_S16, OUT_F16), (PCM_S16, OUT_BF16), (PCM_F32, OUT_F16)], ids=["s16-f16", "s16-bf16", "f32-f16"])
@pytest.mark.parametrize("mode", [None, "f32"], ids=["f64", "f32"])
def test_16_bit_ends(jfk, mode, pcm, out):
    s16 = s16_clips(jfk, PADDED)
    clips = s16 if pcm == PCM_S16 else [to_f32(c) for c in s16]
    flat, offs, lens = lay_out(clips, np.int16 if pcm == PCM_S16 else np.float32, [1 + i % 3 for i in range(len(clips))])
    assert {int(o) & 1 for o in offs} == {0, 1}, "clips at odd and even samples"
    flat32, offs32, lens32 = lay_out([to_f32(c) for c in s16], np.float32, [1 + i % 3 for i in range(len(clips))])
    mel = make(80, mode)
    d, d32 = dev(flat), dev(flat32)
    _, g32 = both(mel, d32.ptr, offs32, lens32, 4800, "the f32 split call", split=True)
    for shift in (0, 1):                                     # 1: the output starts at an odd 16-bit element
        for mel_major in (True, False):
            both(mel, d.ptr, offs, lens, 4800, f"({pcm}, {out}) mel_major {mel_major} shift {shift}", pcm=pcm, out=out, mel_major=mel_major, shift=shift)
        _, g = both(mel, d.ptr, offs, lens, 4800, f"({pcm}, {out}) split shift {shift}", pcm=pcm, out=out, split=True, shift=shift)
        assert np.array_equal(g, g32), "d_clip_max differs from the f32 split call's bits"
    d.free(); d32.free(); mel.close()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(oracle):
    from mel_spec_amd import _lib
    L = _lib.lib()
    clips = [noise(1, 4800, oracle), noise(2, 1234, oracle)]
    flat, offs, lens = lay_out(clips, np.float32, [1, 2])
    d, t_off, t_len = dev(flat), dev(offs, np.uint64), dev(lens, np.uint64)

    def refused(mel, kind, pad_to=4800, n=2, null=(), pcm=PCM_F32, out=OUT_F16, misalign=None):
        f, mx = Fence(2 * 30 * 128, (out if out in (OUT_F32, OUT_F16, OUT_BF16) else OUT_F16) if "io" in kind else OUT_F32), Fence(2, OUT_F32)          # an unknown code: any fence will do
        vp = lambda name, p: None if name in null else C.c_void_p(p + (1 if misalign == name else 0))
        a = [mel._h, vp("pcm", d.ptr)] + ([pcm] if "io" in kind else []) + [vp("offs", t_off.ptr), vp("lens", t_len.ptr), n, pad_to, vp("dst", f.ptr)] + ([out] if "io" in kind else [])
        a += [None] + ([vp("max", mx.ptr)] if "split" in kind else [1]) + [None]
        rc = getattr(L, "melspec_whisper_compute_ragged_device_desc" + kind)(*a)
        mel.synchronize()
        bits, g = f.bits(), mx.bits()
        assert np.all(bits == f.s) and np.all(g == mx.s), f"a refused call wrote {int((bits != f.s).sum()) + int((g != mx.s).sum())} elements"
        f.free(); mx.free()
        return rc

    kinds = ("", "_split", "_io", "_split_io")
    other = M.HipMelSpectrogram(512, 160, 16000.0, 80, device=0)
    assert L.melspec_whisper_supports_desc(other._h) == 0 and not M.supports_whisper_desc(other)
    for kind in kinds:
        assert refused(other, kind) == ERR_UNSUPPORTED and "n_fft = 512" in _lib.last_error()
        assert refused(other, kind, pad_to=0, n=0, null=("pcm", "offs", "lens", "dst", "max")) == ERR_UNSUPPORTED          # before everything but the context and the codes
    assert refused(other, "_io", pcm=7) == ERR_INVALID_ARG and refused(other, "_split_io", out=9) == ERR_INVALID_ARG
    other.close()
    mel = make(80)
    assert L.melspec_whisper_supports_desc(mel._h) == 1
    for kind in kinds:
        assert refused(mel, kind, pad_to=0) == ERR_INVALID_ARG and "fixed width" in _lib.last_error()
        assert refused(mel, kind, pad_to=399) == ERR_INVALID_ARG and "400" in _lib.last_error()
        assert refused(mel, kind, pad_to=0, n=0) == ERR_INVALID_ARG                      # pad_to before the clip count
        assert refused(mel, kind, n=0) == 0
        assert refused(mel, kind, n=0, null=("pcm", "offs", "lens", "dst", "max")) == 0          # ... which comes before the pointers
        for ptr in ("offs", "lens", "pcm", "dst"):
            assert refused(mel, kind, null=(ptr,)) == ERR_INVALID_ARG and "NULL" in _lib.last_error(), (kind, ptr)
    for kind in ("_split", "_split_io"):
        assert refused(mel, kind, null=("max",)) == ERR_INVALID_ARG and "d_clip_max" in _lib.last_error()
    for kind in ("_io", "_split_io"):
        assert refused(mel, kind, pcm=2) == ERR_INVALID_ARG and "pcm_dtype" in _lib.last_error()
        assert refused(mel, kind, out=3) == ERR_INVALID_ARG and "out_dtype" in _lib.last_error()
        assert refused(mel, kind, pcm=7, pad_to=0, null=("pcm",)) == ERR_INVALID_ARG and "pcm_dtype" in _lib.last_error()       # the codes come first
        assert refused(mel, kind, misalign="dst") == ERR_INVALID_ARG and "aligned" in _lib.last_error()
        assert refused(mel, kind, pcm=PCM_S16, misalign="pcm") == ERR_INVALID_ARG and "aligned" in _lib.last_error()
    for b in (d, t_off, t_len):
        b.free()
    mel.close()


# ---- 9. Python on real audio --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_python_function_on_jfk_in_five_pieces(jfk, n_mels):
    cuts = [0, 30001, 30001 + 16000, 90000, 130007, len(jfk)]
    offs = np.array(cuts[:-1], np.uint64)
    lens = np.array([b - a for a, b in zip(cuts[:-1], cuts[1:])], np.uint64)
    mel = make(n_mels)
    want = M.whisper_features_batch(mel, [jfk[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    d, t_off, t_len = dev(jfk), dev(offs), dev(lens)
    out = Fence(5 * 3000 * n_mels, OUT_F32)
    M.whisper_ragged_device_desc(mel, d.ptr, t_off.ptr, t_len.ptr, 5, out.ptr)          # pad_to = 480000, mel-major
    mel.synchronize()
    got = as_f32(out.bits()).reshape(5, n_mels, 3000)
    for i in range(5):
        assert want[i].shape == (n_mels, 3000) and np.array_equal(got[i], want[i]), f"piece {i}"
    for b in (d, t_off, t_len, out):
        b.free()
    mel.close()
