"""fbank512_clip_kernel on many tiny clips: every clip of every batch, in fenced outputs.

The kernel's eight waves synchronise across clips without a barrier (csrc/fbank512_kernels.hpp: per-wave column sums in part[2][8][96],
an arrival counter that elects the wave that folds them, ready[2] / mean[2], all double-buffered by clip parity; ragged batches hand the
clips out through a ring of eight ids).  The other fbank tests give a workgroup two or three well-balanced clips.  Here a parity slot is
reused while some waves have no work at all: clips of fewer than eight units (a wave whose share of the units is empty goes straight to
the arrival), three to five clips per workgroup, and ragged batches that end in a long run of clips without a frame.

References, none of them the kernel under test: the oracle (with apply_cmn = 0 for the rows before CMN), and the project's other kernel
pair -- the same clips in launches too small for the clip kernel (fused wave kernel + cmn_kernel), whose bits a clip must keep whatever
batch it is in.  The CPU test at the end keeps the Python mirror of the host's two dispatch rules in step with fused512_route.hpp and
fbank512.hip."""
import os
import re

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_whole_batch import Fence, _compare, _cus, _no_sentinel, _noise, _pmap, _upload, run_ragged, SENTINEL, THREADS, TOL

FL, FS, FPU, WAVES = 400, 160, 4, 8      # frame length, shift (16 kHz), frames per unit (kFbFPW), waves of the clip kernel
SMALL = 40                               # clips per launch of the two-kernel reference path (fewer than any CU count here)


# ---- the host's dispatch rules, mirrored (fused512_route.hpp: clip_shape_ok, clip_uniform_ok, clip_ragged_ok) ----------------------

def takes_clip_kernel_uniform(n_clips, cus, n_mels):
    """a uniform batch with CMN (power spectra, aligned output) runs on fbank512_clip_kernel"""
    passes = (n_clips + cus - 1) // cus
    return n_mels % 4 == 0 and n_mels <= 89 and n_clips >= cus and n_clips * 100 >= passes * cus * 85


def takes_clip_kernel_ragged(frames, cus, n_mels=80):
    """a ragged batch (outputs at multiples of four floats) is handed out by clip"""
    return n_mels % 4 == 0 and n_mels <= 89 and len(frames) >= 2 * cus and max(frames) * 2 * cus <= sum(frames)


def shares(frames):
    """units of each of the eight waves (u1 - u0 of the kernel)"""
    units = (frames + FPU - 1) // FPU
    return [units * (w + 1) // WAVES - units * w // WAVES for w in range(WAVES)]


# ---- A1: the matrix ---------------------------------------------------------------------------------------------------------------

F_SWEEP = (1, 2, 4, 5, 9, 13, 27, 29, 33, 36)     # units 1, 1, 1, 2, 3, 4, 7, 8, 9, 9
COUNTS = {"3cus": lambda cus: 3 * cus, "4cus": lambda cus: 4 * cus, "5cus-": lambda cus: 5 * cus - cus // 8}
# (n_mels, frames per clip, clip count, samples past the last frame)
A1_CASES = ([(80, F, k, 0) for F in F_SWEEP for k in COUNTS]
            + [(nm, F, "5cus-", 0) for nm in (40, 24) for F in (1, 5, 29, 33)]        # LensKaldi40, LensRuntime
            + [(80, 13, "3cus", 77), (40, 2, "4cus", 77)])


def _case_id(c):
    return f"m{c[0]}-F{c[1]}-{c[2]}" + (f"+{c[3]}" if c[3] else "")


class Batch:
    """the clips of one A1 case on the device, and both oracles"""

    def __init__(self, gpu, oracle, case):
        self.nm, self.F, kind, extra = case
        self.cus = _cus()
        self.n_clips = COUNTS[kind](self.cus)
        self.n = FL + (self.F - 1) * FS + extra
        assert takes_clip_kernel_uniform(self.n_clips, self.cus, self.nm), (self.n_clips, self.cus)
        assert not takes_clip_kernel_uniform(SMALL, self.cus, self.nm)
        self.clips = _noise(self.n_clips, self.n, 6000 + 37 * self.F)
        self.pcm = _upload(gpu, self.clips)
        self.gpu, self.oracle = gpu, oracle

    def want(self, apply_cmn):
        oc = self.oracle.fbank_default_config()
        oc.num_mel_bins, oc.apply_cmn = self.nm, int(apply_cmn)
        return self.oracle.fbank_batch(self.clips, oc, THREADS)

    def context(self, **kw):
        fb = self.gpu.Fbank(self.gpu.FbankConfig(num_mel_bins=self.nm, **kw))
        assert fb.uses_fast_path and fb.num_frames(self.n) == self.F
        return fb

    def fused(self, fb, per_launch=None):
        """compute_uniform_device of the whole batch, in launches of per_launch clips -> bits [clip][frame][mel]"""
        per = per_launch or self.n_clips
        out = Fence(self.gpu, self.n_clips * self.F * self.nm)
        for c0 in range(0, self.n_clips, per):
            k = min(per, self.n_clips - c0)
            fb.compute_uniform_device(self.pcm.ptr + c0 * self.n * 4, self.n, self.n, k, out.ptr + c0 * self.F * self.nm * 4)
        fb.synchronize()
        bits = out.bits()
        _no_sentinel(bits, "rows")
        return bits.reshape(self.n_clips, self.F, self.nm)

    def split(self, fb):
        rows, means = Fence(self.gpu, self.n_clips * self.F * self.nm), Fence(self.gpu, self.n_clips * self.nm)
        fb.compute_uniform_device_split(self.pcm.ptr, self.n, self.n, self.n_clips, rows.ptr, means.ptr)
        fb.synchronize()
        rb, mb = rows.bits(), means.bits()
        _no_sentinel(rb, "split rows")
        _no_sentinel(mb, "split means")
        return rb.reshape(self.n_clips, self.F, self.nm), mb.reshape(self.n_clips, 1, self.nm)

    def facts(self):
        return f"clips={self.n_clips} ({self.n_clips / self.cus:.3f}/CU) frames={self.F} shares={shares(self.F)}"


def _f32(bits):
    return bits.view(np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", A1_CASES, ids=_case_id)
def test_tiny_uniform_fused_cmn(gpu, oracle, case):
    """CMN inside: every clip within 1e-4 of the oracle; the bits of the same clips in launches of 40 (wave kernel + cmn_kernel); the same
    bits on a second run"""
    b = Batch(gpu, oracle, case)
    fb = b.context()
    got = b.fused(fb)
    worst = _compare(list(_f32(got)), list(b.want(True)), TOL, f"fused {_case_id(case)}")
    print(f"\nTINY-CLIPS fused {_case_id(case)}: {b.facts()} worst={worst:.3e}")
    small = b.fused(fb, SMALL)
    diff = np.flatnonzero(np.any(got != small, axis=(1, 2)))
    assert diff.size == 0, f"{diff.size} clips differ from the two-kernel path's bits, first clip {int(diff[0])}"
    again = b.fused(fb)
    diff = np.flatnonzero(np.any(got != again, axis=(1, 2)))
    assert diff.size == 0, f"{diff.size} clips differ on the second run, first clip {int(diff[0])}"
    b.pcm.free()
    fb.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", A1_CASES, ids=_case_id)
def test_tiny_uniform_split(gpu, oracle, case):
    """The split output: rows = the apply_cmn = false output bit for bit and within 1e-4 of the oracle's; every mean written; rows - means
    in f32 = the fused output bit for bit; and the means on their own against the f64 column mean of the oracle's rows.  (For a clip of
    one frame rows - means is 0 whatever the mean is: only the last gate sees a wrong mean there.)  The bound of that gate: the rows are
    within 1e-4 of the oracle's, so is their exact mean; an f32 sum of F <= 36 terms of magnitude <= M in any order plus one division adds
    less than F x 2^-24 x M."""
    b = Batch(gpu, oracle, case)
    fb = b.context()
    rows, means = b.split(fb)
    tag = _case_id(case)
    raw = b.context(apply_cmn=False)
    plain = b.fused(raw)
    raw.close()
    diff = np.flatnonzero(np.any(rows != plain, axis=(1, 2)))
    assert diff.size == 0, f"{diff.size} clips' rows differ from the apply_cmn = false output, first clip {int(diff[0])}"
    want_rows = b.want(False)
    worst_rows = _compare(list(_f32(rows)), list(want_rows), TOL, f"split rows {tag}")
    # the means on their own
    M = np.maximum(np.abs(_f32(rows)).max(axis=(1, 2)), np.abs(want_rows).max(axis=(1, 2))).astype(np.float64)
    bound = TOL + b.F * 2.0 ** -24 * M
    want_means = want_rows.astype(np.float64).mean(axis=1, keepdims=True)
    d = np.abs(_f32(means).astype(np.float64) - want_means)
    d[np.isnan(d)] = np.inf
    worst_means = float(d.max())
    print(f"\nTINY-CLIPS split {tag}: {b.facts()} worst rows={worst_rows:.3e} worst means={worst_means:.3e} "
          f"(bound {float(bound.min()):.3e} .. {float(bound.max()):.3e})")
    bad = np.flatnonzero(d.max(axis=(1, 2)) > bound)
    assert bad.size == 0, f"{bad.size} of {b.n_clips} clips' means are off by more than 1e-4 + F 2^-24 max|row|: first clip {int(bad[0])} " \
                          f"(workgroup {int(bad[0]) % b.cus}, its clip no. {int(bad[0]) // b.cus}) by {float(d[bad[0]].max()):.3e}; worst {worst_means:.3e}"
    # rows - means = what the CMN inside stores
    fused = b.fused(fb)
    sub = (_f32(rows) - _f32(means)).astype(np.float32).view(np.uint32)
    diff = np.flatnonzero(np.any(sub != fused, axis=(1, 2)))
    assert diff.size == 0, f"{diff.size} clips: rows - means differs from the fused output, first clip {int(diff[0])}"
    b.pcm.free()
    fb.close()


# ---- A2: ragged by clip, tiny clips, a long tail of clips without a frame ---------------------------------------------------------

def ragged_tiny_batch(cus, K, seed=23):
    """5 x cus clips of 1 .. 36 frames (with runs of equal lengths) and K clips without a frame scattered through them -> clip lengths"""
    rng = np.random.default_rng(seed)
    n_real = 5 * cus
    frames = rng.integers(1, 37, n_real)
    frames[100:140] = 17                      # ties in the longest-first order
    frames[300:330] = 36
    frames[n_real - 25:n_real - 5] = 1
    lens = [FL + (int(f) - 1) * FS + int(j) for f, j in zip(frames, rng.integers(0, FS, n_real))]
    where = sorted(set(int(v) for v in np.linspace(3, n_real - 2, K))) if K else []
    assert len(where) == K
    for i, at in enumerate(reversed(where)):  # (from the back: the earlier positions stay put)
        lens.insert(at, (0, 1, FL - 1)[i % 3])
    return lens


def _frames_of(n):
    return 0 if n < FL else 1 + (n - FL) // FS


@pytest.mark.gpu
@pytest.mark.parametrize("gaps", [False, True], ids=["packed", "gapped"])
@pytest.mark.parametrize("K", [0, 9, 64])
def test_tiny_ragged_by_clip(gpu, oracle, K, gaps):
    """Every clip within 1e-4 of the oracle; the bits of the same clips in ragged launches too small to go by clip; gaps and the guard
    bands untouched; the same bits on a second run and through the host pipeline (Fbank.compute_many)"""
    cus = _cus()
    fb = gpu.Fbank()
    nm = fb.num_mel_bins
    lens = ragged_tiny_batch(cus, K)
    frames = [fb.num_frames(n) for n in lens]
    assert frames == [_frames_of(n) for n in lens] and frames.count(0) == K and len(lens) == 5 * cus + K
    assert takes_clip_kernel_ragged(frames, cus, nm), (len(frames), max(frames), sum(frames))
    base = _noise(len(lens), max(lens), 8000)
    clips = [x[:n] for x, n in zip(base, lens)]
    oc = oracle.fbank_default_config()
    want = _pmap(lambda x: oracle.fbank_compute(x, oc), clips)
    got = run_ragged(gpu, fb, np.concatenate(clips), lens, frames, nm, gaps)
    worst = _compare(got, want, TOL, f"ragged K={K}")
    print(f"\nTINY-CLIPS ragged K={K} {'gapped' if gaps else 'packed'}: clips={len(lens)} ({len(lens) / cus:.3f}/CU) frames={sum(frames)} "
          f"longest={max(frames)} frameless={K} worst={worst:.3e}")
    step = cus + cus // 2                     # fewer than 2 x cus clips: the fused wave kernel + cmn_kernel
    for c0 in range(0, len(lens), step):
        sl = slice(c0, c0 + step)
        assert not takes_clip_kernel_ragged(frames[sl], cus, nm)
        small = run_ragged(gpu, fb, np.concatenate(clips[sl]), lens[sl], frames[sl], nm, gaps)
        for i, (a, s) in enumerate(zip(got[sl], small)):
            assert np.array_equal(a.view(np.uint32), s.view(np.uint32)), f"clip {c0 + i} ({frames[c0 + i]} frames) differs from its bits in a small launch"
    again = run_ragged(gpu, fb, np.concatenate(clips), lens, frames, nm, gaps)
    for i, (a, s) in enumerate(zip(got, again)):
        assert np.array_equal(a.view(np.uint32), s.view(np.uint32)), f"clip {i} differs on the second run"
    if not gaps:
        many = fb.compute_many(clips)
        for i, (a, s) in enumerate(zip(got, many)):
            assert a.shape == s.shape and np.array_equal(a.view(np.uint32), s.view(np.uint32)), f"clip {i} differs through compute_many"
    fb.close()


# ---- A3: either side of the dispatch threshold; a split call without a frame -------------------------------------------------------

@pytest.mark.gpu
def test_tiny_one_frame_clips_either_side_of_the_threshold(gpu, oracle):
    """cus - 1 one-frame clips (wave kernel + cmn_kernel) and cus of them (clip kernel): the same bits, all 0.0 after CMN, the means the
    rows themselves"""
    cus = _cus()
    assert not takes_clip_kernel_uniform(cus - 1, cus, 80) and takes_clip_kernel_uniform(cus, cus, 80)
    fb = gpu.Fbank()
    clips = _noise(cus, FL, 9100)
    pcm = _upload(gpu, clips)
    outs = []
    for n_clips in (cus - 1, cus):
        out, rows, means = Fence(gpu, n_clips * 80), Fence(gpu, n_clips * 80), Fence(gpu, n_clips * 80)
        fb.compute_uniform_device(pcm.ptr, FL, FL, n_clips, out.ptr)
        fb.compute_uniform_device_split(pcm.ptr, FL, FL, n_clips, rows.ptr, means.ptr)
        fb.synchronize()
        ob, rb, mb = out.bits(), rows.bits(), means.bits()
        for x, what in ((ob, "rows"), (rb, "split rows"), (mb, "split means")):
            _no_sentinel(x, what)
        assert not ob.any(), f"{int(np.count_nonzero(ob))} values of one-frame clips are not +0.0 after CMN"
        assert np.array_equal(rb, mb), "the mean of one row is not the row"
        outs.append(rb.reshape(n_clips, 1, 80))
    assert np.array_equal(outs[0], outs[1][:cus - 1]), "a clip's bits depend on the side of the dispatch threshold"
    oc = oracle.fbank_default_config()
    oc.apply_cmn = 0
    worst = _compare(list(_f32(outs[1])), list(oracle.fbank_batch(clips, oc, THREADS)), TOL, "one-frame clips")
    print(f"\nTINY-CLIPS threshold: clips={cus - 1}, {cus} frames=1 worst={worst:.3e}")
    pcm.free()
    fb.close()


@pytest.mark.gpu
def test_tiny_split_without_a_frame(gpu):
    """clips shorter than a frame: no rows (the buffer stays untouched), the mean of nothing is reported as 0.0"""
    fb = gpu.Fbank()
    n_clips = _cus() + 3
    assert fb.num_frames(FL - 1) == 0
    pcm = _upload(gpu, np.ones(n_clips * (FL - 1), np.float32))
    rows, means = Fence(gpu, 4096), Fence(gpu, n_clips * 80)
    fb.compute_uniform_device_split(pcm.ptr, FL - 1, FL - 1, n_clips, rows.ptr, means.ptr)
    fb.synchronize()
    rb, mb = rows.bits(), means.bits()
    assert np.all(rb == SENTINEL), "rows were written for clips without a frame"
    assert not mb.any(), "the means of clips without a frame are not +0.0"
    print(f"\nTINY-CLIPS no-frame split: clips={n_clips} frames=0 worst=0.000e+00")
    pcm.free()
    fb.close()


# ---- C: the mirror against the source (CPU) ---------------------------------------------------------------------------------------

def _host_source(name="fbank512.hip"):
    return open(os.path.join(ROOT, "mel_spec_amd", "csrc", name)).read()


def _body(src, head):
    """the text of the function that begins with `head`, white space folded"""
    body = src[src.index(head):]
    return re.sub(r"\s+", " ", body[:body.index("\n}\n")])


def test_tiny_clips_dispatch_mirror_matches_the_host():
    """the constants takes_clip_kernel_uniform / _ragged rely on are still in the host's rules (fused512_route.hpp; the alignment of the
    output offsets in fbank512.hip), and the A1 matrix reaches the clip kernel on any CU count"""
    route = _host_source("fused512_route.hpp")
    shape = _body(route, "constexpr bool clip_shape_ok(const Fused512Shape &s, int nm) {")
    for piece in ("nm % 4 == 0", "nm <= 89"):
        assert piece in shape, f"clip_shape_ok no longer holds `{piece}`"
    uniform = _body(route, "constexpr bool clip_uniform_ok(uint32_t n_clips, uint32_t cus) {")
    for piece in ("n_clips >= cus", "passes = (n_clips + cus - 1) / cus",
                  "static_cast<uint64_t>(n_clips) * 100 >= static_cast<uint64_t>(passes) * cus * 85"):
        assert piece in uniform, f"clip_uniform_ok no longer holds `{piece}`"
    rag = _body(route, "constexpr bool clip_ragged_ok(uint32_t n_clips, uint32_t cus, uint64_t longest, uint64_t total) {")
    for piece in ("n_clips >= 2u * cus", "longest * 2 * static_cast<uint64_t>(cus) <= total"):
        assert piece in rag, f"clip_ragged_ok no longer holds `{piece}`"
    # both entry points ask the shared rules, with the object's CU count
    launch = _body(_host_source(), "static int fbank_launch(melspec_fbank *fb, const BatchPlan &pl, uint32_t n_clips, uint64_t fpc, hipStream_t s, int io = 0,")
    for piece in ("cus = static_cast<uint32_t>(fb->dev.cus)", "clip_shape_ok(shape, nm)", "clip_uniform_ok(n_clips, cus)"):
        assert piece in launch, f"fbank_launch no longer holds `{piece}`"
    ragged = _body(_host_source(), "static int fbank_ragged(melspec_fbank *fb")
    for piece in ("clip_shape_ok(fbank_shape(fb), nm)", "clip_ragged_ok(n_clips, static_cast<uint32_t>(fb->dev.cus), longest, total)", "h_out_offsets[i] % 4 == 0"):
        assert piece in ragged, f"fbank_ragged no longer holds `{piece}`"
    csrc = os.path.join(ROOT, "mel_spec_amd", "csrc")
    assert "constexpr int WAVES = 8, NT = WAVES * 64;" in open(os.path.join(csrc, "fbank512_kernels.hpp")).read()
    assert re.search(r"constexpr int kFbFPW = 4;", open(os.path.join(csrc, "fbank_wave.hpp")).read())
    for cus in (256, 304, 64):
        for nm, F, kind, _ in A1_CASES:
            n = COUNTS[kind](cus)
            assert takes_clip_kernel_uniform(n, cus, nm), (cus, nm, F, kind)
            assert n // cus >= 3, (cus, kind)                      # a parity slot is reused
        assert not takes_clip_kernel_uniform(SMALL, cus, 80) and SMALL < cus
        assert not takes_clip_kernel_uniform(cus - 1, cus, 80) and takes_clip_kernel_uniform(cus, cus, 80)
        assert not takes_clip_kernel_uniform(4 * cus + 1, cus, 80)        # 85 %: a fifth pass of one clip
        assert not takes_clip_kernel_uniform(3 * cus, cus, 82) and not takes_clip_kernel_uniform(3 * cus, cus, 92)
        for K in (0, 9, 64):
            frames = [_frames_of(n) for n in ragged_tiny_batch(cus, K)]
            assert len(frames) == 5 * cus + K and frames.count(0) == K and max(frames) == 36
            assert takes_clip_kernel_ragged(frames, cus)
            assert not takes_clip_kernel_ragged(frames[:cus + cus // 2], cus)
    # the shares the sweep is there for: empty ones below eight units, uneven ones above
    assert [sum(1 for s in shares(F) if s == 0) for F in F_SWEEP] == [7, 7, 7, 6, 5, 4, 1, 0, 0, 0]
    assert shares(33) == shares(36) == [1, 1, 1, 1, 1, 1, 1, 2]
