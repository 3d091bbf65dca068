"""pow2_frame_kernel and generic_frame_kernel past one trip of their grids -- every frame of every clip against the oracle, in fenced
output buffers, in the Whisper, Kaldi and NeMo flavours.

Every geometry off the fused 400- and 512-point kernels turns PCM into rows on one of these two (generic_kernels.hpp, pow2.hip).  Both
are persistent: launch_pow2 starts min(groups, CUs) workgroups of up to kMaxWaves waves, a wave owns FW frames per iteration and walks
the batch with a stride of grid x waves x FW frames; generic_frame_kernel starts at most 8 x CUs workgroups and strides by the grid.
tests/test_whole_batch.py and tests/test_gpu_parity.py give them a few hundred frames: the first iteration of the frame loop.  The
second one is where pow2_frame_kernel has its logic -- advance() (a uniform batch walked without a division: step_clips, step_rest, one
conditional wrap, `have`, `real`), the frame fetched one iteration ahead (kAhead: cur = nxt, raw = nraw) or the tail without it
(cur = advance(cur, base); fetch), the reuse of a frame's LDS region (acc cleared per frame, the power row over the points at
M >= 1024), the zero columns of the layouts and of NeMo's pad_to written by `have && !real` frames on a later trip, and
place() -> locate_unit on every trip of a ragged batch.

The real waves per workgroup depend on the bank (pow2_lds), which the tests do not restate: a batch is sized by the upper bound
S_max = CUs x kMaxWaves x FW, and T = 2 S_max + S_max / 2 + 3 frames take at least three trips with a partial last one for ANY waves per
workgroup from 1 to kMaxWaves (fewer waves: more trips; the CPU test at the end checks it for four CU counts).  Clip shapes:

  short      many clips of 37 or 41 frames: step_clips large, step_rest != 0, trip boundaries inside clips
  one-frame  clips of exactly n_fft samples: units_per_clip == 1, every frame slot of a wave holds another clip
  long       three clips of about 0.85 S_max frames: step_clips 0 or 1, step_rest nearly a whole clip
  layout     the short shape through compute_uniform_device_interleaved, min_width = frames + 41: units_per_clip is the width, and
             the zero columns fall in later trips
  ragged     ragged_lengths, enough clips for 2 S_max + 1 frames: place() on every trip

Every GPU test asserts: guard bands intact, no sentinel left where a frame belongs, the gaps between ragged outputs untouched, layout and
pad_to padding exactly 0.0, and EVERY frame of EVERY clip at the gate the project already uses for the path: 2e-6 (F64_TOL) for the
Whisper flavour on these f64 kernels, 1e-4 (TOL) for Kaldi against oracle.fbank_batch / fbank_compute and for NeMo against
oracle.blm_compute(x, cfg, True), 2e-5 between pow2_frame_kernel and generic_frame_kernel (test_pow2_kernel_kaldi_rates_...).

Position independence, bit for bit: in every uniform short / one-frame / layout batch three clips that start past the second
trip are copies of clips 0, 1 and 2, and their rows -- finished rows where CMN or normalisation is on -- must be the originals' bits.
That is the check that sees state carried from one iteration of the frame loop into the next at sizes below any tolerance."""
import os
import re

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from conftest import ROOT
from test_stft_whole_batch import check_generic_batch, generic_batch
from test_whole_batch import (F64_TOL, GENERIC, POW2, SENTINEL, SR, THREADS, TOL, Fence, _compare, _cus, _no_sentinel, _noise, _pmap, _upload,
                              mel_oracle, ragged_lengths, run_interleaved, run_ragged, run_ragged_desc, run_uniform)

CROSS_TOL = 2e-5      # pow2_frame_kernel against generic_frame_kernel: the f32 logarithm of the one against the f64 one of the other

# Pow2Shape<LOGM> (mel_spec_amd/csrc/pow2_wave.hpp) and launch_pow2 (mel_spec_amd/csrc/pow2.hip), by n_fft:
#   M = n_fft / 2, LOGM = log2 M;  LF = M >= 512 ? 64 : M / 8 lanes per frame;  FW = 64 / LF frames per wave;
#   kMaxWaves = MS_POW2_MAXW (8) up to M = 512, MS_POW2_MAXWH (6) for M = 1024 as two halves (MS_POW2_HALVES 1; MS_POW2_MAXW16 otherwise).
# n_fft -> (LOGM, LF, FW, kMaxWaves); test_pow2_shape_table_is_the_sources keeps it in step with the two files.
POW2_SHAPE = {128: (6, 8, 8, 8), 256: (7, 16, 4, 8), 512: (8, 32, 2, 8), 1024: (9, 64, 1, 8), 2048: (10, 64, 1, 6)}
CU_COUNTS = (64, 228, 256, 304)


# ---- the batch recipes (arithmetic on the CU count only: the CPU test at the end restates them) ------------------------------------

def s_max(n_fft, cus):
    """the frames of one trip of a full grid at the most waves a workgroup can have"""
    _, _, fw, max_waves = POW2_SHAPE[n_fft]
    return cus * max_waves * fw


def strides(n_fft, cus):
    """the stride of the frame loop for every waves per workgroup launch_pow2 can pick (grid = CUs: the batches below have more groups)"""
    _, _, fw, max_waves = POW2_SHAPE[n_fft]
    return [cus * w * fw for w in range(1, max_waves + 1)]


def min_units(n_fft, cus):
    S = s_max(n_fft, cus)
    return 2 * S + S // 2 + 3


def trips_ok(n_units, n_fft, cus):
    """at least three trips and a partial last one, whatever the waves per workgroup"""
    return all(n_units > 2 * st and n_units % st != 0 for st in strides(n_fft, cus))


def pow2_batch(shape, n_fft, cus, frames=37, units_per_clip=None):
    """-> (n_clips, frames per clip, units per clip, the clips that are copies of clips 0, 1, 2) of a uniform batch of
    pow2_frame_kernel; units_per_clip: the output width where it is not the frames (layouts, pad_to)"""
    S, T = s_max(n_fft, cus), min_units(n_fft, cus)
    if shape == "long":                    # three clips of about 0.85 S_max frames
        f = -(-85 * S // 100)
        while not (3 * f >= T and trips_ok(3 * f, n_fft, cus)):
            f += 1
        return 3, f, f, ()
    upc = 1 if shape == "one-frame" else (units_per_clip or frames)
    f = 1 if shape == "one-frame" else frames
    first = -(-2 * S // upc)               # the first clip that starts past the second trip, at any waves per workgroup
    n_clips = max(-(-T // upc), first + 4)
    while not trips_ok(n_clips * upc, n_fft, cus):
        n_clips += 1
    return n_clips, f, upc, (first + 1, first + 2, first + 3)


def check_recipe(n_clips, upc, dups, n_fft, cus, walked=True):
    """what a GPU test asserts of its own batch before it runs it"""
    total = n_clips * upc
    assert total >= min_units(n_fft, cus) and trips_ok(total, n_fft, cus), (n_clips, upc, cus)
    if walked and upc > 1:                 # advance(): a step that is no whole number of clips
        assert all(st % upc != 0 for st in strides(n_fft, cus)), (upc, cus)
    for d in dups:
        assert 2 < d < n_clips and d * upc >= 2 * s_max(n_fft, cus), (d, n_clips, upc, cus)
    return dict(units=total, s_max=s_max(n_fft, cus), trips_at_max_waves=-(-total // s_max(n_fft, cus)))


def generic_layout_batch(cus, width):
    """about 2.3 trips of generic_frame_kernel's 8 x CUs workgroups, in clips of `width` units"""
    return int(2.3 * 8 * cus) // width + 1


def ragged_batch(n_fft, frame_len, hop, n_max, cus, seed):
    """ragged_lengths with enough clips for 2 S_max + S_max / 2 + 3 frames -> (clip lengths, frames per clip)"""
    n_clips = 64
    while True:
        lens = ragged_lengths(frame_len, hop, n_clips, n_max, seed)
        frames = [0 if n < frame_len else 1 + (n - frame_len) // hop for n in lens]
        if sum(frames) >= min_units(n_fft, cus) and trips_ok(sum(frames), n_fft, cus):
            return lens, frames
        n_clips += 16


# ---- the checks of this file -------------------------------------------------------------------------------------------------------

def check_copies(got, dups, what):
    """clip dups[k] was given clip k's samples: its rows are clip k's bit for bit"""
    for k, d in enumerate(dups):
        a = np.ascontiguousarray(got[k]).view(np.uint32)
        b = np.ascontiguousarray(got[d]).view(np.uint32)
        assert a.shape == b.shape, (what, k, d, a.shape, b.shape)
        diff = a != b
        assert not diff.any(), f"{what}: clip {d}, a copy of clip {k}, differs from it in {int(diff.sum())} words " \
                               f"(first at (frame, mel) = {tuple(int(v) for v in np.argwhere(diff)[0])}): the result depends on the clip's position"


def check_padding(pad, want, what):
    """pad_to columns: the oracle's, and exactly 0.0"""
    assert pad.shape == want.shape, (what, pad.shape, want.shape)
    assert np.array_equal(pad, want), f"{what}: {int(np.sum(pad != want))} padding values differ from the oracle's"
    assert np.all(pad == 0.0), f"{what}: {int(np.sum(pad != 0.0))} padding values are not 0.0"


def compare_all(got, want, tol, what):
    """_compare on the clips of a uniform batch as one array (tens of thousands of one-frame clips): the index it reports is
    (0, clip, frame, mel)"""
    return _compare([np.stack(got)], [np.stack(want)], tol, what + " [index: 0, clip, frame, mel]")


_REF = {}


def _once(key, make):
    """a reference is computed once, shared by the two passes of a test, and read-only"""
    if key not in _REF:
        v = make()
        for a in v:
            a.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def with_copies(clips, dups):
    for k, d in enumerate(dups):
        clips[d] = clips[k]
    return clips


# ---- 1. pow2_frame_kernel, Whisper flavour -----------------------------------------------------------------------------------------

W128, W256, W512, W1024, W2048 = (128, 32, 8000.0, 20), (256, 64, 8000.0, 40), (512, 160, SR, 200), (1024, 256, SR, 80), (2048, 512, 44100.0, 128)
# id, geometry, shape, entry, frames per clip of the short shape, first clip of the content
WHISPER_CASES = [
    ("128-short", W128, "short", "uniform", 37, 100000),         # FW = 8: eight clips' frames in one wave, prefetching
    ("128-one-frame", W128, "one-frame", "uniform", 1, 200000),
    ("256-short", W256, "short", "uniform", 41, 300000),
    ("256-padded", W256, "short", "padded", 37, 400000),
    ("512-long", W512, "long", "uniform", 0, 500000),
    ("1024-short", W1024, "short", "uniform", 37, 600000),       # the power row over the points
    ("1024-melmajor", W1024, "short", "melmajor", 41, 700000),
    ("2048-short", W2048, "short", "uniform", 41, 800000),       # kHalves: fetched per half, the tail without the prefetch
    ("2048-long", W2048, "long", "uniform", 0, 900000),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", WHISPER_CASES, ids=lambda c: c[0])
def test_pow2_whisper_whole_batch(gpu, oracle, case):
    cid, geo, shape, entry, frames, seed = case
    cus = _cus()
    fft, hop, sr, nm = geo
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    assert m.plain_kernel_name() == POW2[POW2_SHAPE[fft][0]], m.plain_kernel_name()
    layout = entry != "uniform"
    n_clips, f, upc, dups = pow2_batch(shape, fft, cus, frames, frames + 41 if layout else None)
    facts = check_recipe(n_clips, upc, dups, fft, cus)
    n = fft + (f - 1) * hop
    assert m.num_frames(n) == f and (not layout or m.interleaved_width(n, f + 41) == upc)
    clips = with_copies(_noise(n_clips, n, seed), dups)
    want = _once(("whisper", cid, cus), lambda: mel_oracle(oracle, clips, geo))
    if layout:
        got = run_interleaved(gpu, m, clips, nm, entry == "padded", f + 41)
    else:
        got = run_uniform(gpu, m, clips, nm)
    worst = compare_all(got, want, F64_TOL, f"pow2 whisper {cid}")
    check_copies(got, dups, f"pow2 whisper {cid}")
    print(f"\nWHOLE-BATCH generic/pow2 whisper-{cid}: {m.plain_kernel_name()} clips={n_clips} frames={n_clips * f} worst={worst:.3e} {facts}")
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["ragged", "ragged_desc"])
def test_pow2_whisper_ragged_whole_batch(gpu, oracle, entry):
    """the clip table of the host call (gaps between the outputs) and of the _desc call (in device memory): locate_unit on every trip"""
    cus = _cus()
    fft, hop, sr, nm = W256
    n_max = fft + 150 * hop
    lens, frames = ragged_batch(fft, fft, hop, n_max, cus, 21)
    total = sum(frames)
    assert total >= 2 * s_max(fft, cus) + 1 and trips_ok(total, fft, cus), (total, s_max(fft, cus))
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    assert m.plain_kernel_name() == POW2[7]
    assert frames == [m.num_frames(n) for n in lens]
    base = _noise(len(lens), n_max, 1000000)
    full = _once(("whisper-ragged", cus), lambda: mel_oracle(oracle, base, W256))
    want = [w[:k] for w, k in zip(full, frames)]
    flat = np.concatenate([b[:n] for b, n in zip(base, lens)])
    if entry == "ragged":
        got = run_ragged(gpu, m, flat, lens, frames, nm)
    else:
        got = run_ragged_desc(gpu, m, flat, lens, frames, nm, slack=5000)
    worst = _compare(got, want, F64_TOL, f"pow2 whisper {entry}")
    print(f"\nWHOLE-BATCH generic/pow2 whisper-256-{entry}: clips={len(lens)} frames={total} s_max={s_max(fft, cus)} worst={worst:.3e}")
    m.close()


# ---- 2. pow2_frame_kernel and generic_frame_kernel, Kaldi flavour ------------------------------------------------------------------

# sample rate -> (fft size, frames per clip of the short shape, first clip of the content); frame lengths 200, 551 and 1103 samples
KALDI = {8000.0: (256, 37, 1100000), 22050.0: (1024, 41, 1200000), 44100.0: (2048, 37, 1300000)}
KALDI_CASES = [("8k", 8000.0, False),          # n_fft 256: no prefetch (the Kaldi framing at n_fft <= 512), cur = advance(cur, base)
               ("22k", 22050.0, False),        # n_fft 1024: the prefetching tail
               ("44k", 44100.0, False),        # n_fft 2048: odd frames of 1103 samples, fetched per half (twice: the mean, then the points)
               ("8k-generic", 8000.0, True)]   # generic_frame_kernel's radix-2 path in this flavour, ten times its grid cap


def _fbank(gpu, oracle, sr):
    cfg = gpu.FbankConfig(sample_rate=sr)
    fb = gpu.Fbank(cfg)
    oc = oracle.fbank_default_config()
    oc.sample_rate = sr
    assert not fb.uses_fast_path and cfg.fft_size() == KALDI[sr][0] and cfg.apply_cmn
    return fb, cfg, oc


@pytest.mark.gpu
@pytest.mark.parametrize("case", KALDI_CASES, ids=lambda c: c[0])
def test_pow2_kaldi_whole_batch(gpu, oracle, case):
    """uniform short batches, CMN on: the finished rows against oracle.fbank_batch; under use_generic(2) the same batch on
    generic_frame_kernel, and the two kernels' rows against each other"""
    cid, sr, on_generic = case
    cus = _cus()
    fft, frames, seed = KALDI[sr]
    fb, cfg, oc = _fbank(gpu, oracle, sr)
    nm = fb.num_mel_bins
    n_clips, f, upc, dups = pow2_batch("short", fft, cus, frames)
    facts = check_recipe(n_clips, upc, dups, fft, cus)
    n = cfg.frame_length_samples() + (f - 1) * cfg.frame_shift_samples()
    assert fb.num_frames(n) == f
    clips = with_copies(_noise(n_clips, n, seed), dups)
    want = _once(("kaldi", sr, cus), lambda: list(oracle.fbank_batch(clips, oc, THREADS)))
    cross = ""
    if on_generic:
        assert n_clips * f > 2 * 8 * cus          # past the second trip of generic_frame_kernel's 8 x CUs workgroups
        fb.use_generic(2)
    got = run_uniform(gpu, fb, clips, nm)
    worst = compare_all(got, want, TOL, f"kaldi {cid}")
    check_copies(got, dups, f"kaldi {cid}")
    if on_generic:
        fb.use_generic(False)
        fast = run_uniform(gpu, fb, clips, nm)
        d = compare_all(fast, got, CROSS_TOL, "kaldi 8k: pow2_frame_kernel against generic_frame_kernel")
        # two transforms and two logarithms (v_log_f32 against f64 log): over 1.6 million values the same bits everywhere would mean
        # that use_generic(2) did not change the kernel
        assert not np.array_equal(np.stack(fast).view(np.uint32), np.stack(got).view(np.uint32)), "use_generic(2) ran the same kernel"
        cross = f" pow2-vs-generic={d:.3e}"
    print(f"\nWHOLE-BATCH generic/pow2 kaldi-{cid}: n_fft={fft} clips={n_clips} frames={n_clips * f} worst={worst:.3e}{cross} {facts}")
    fb.close()


@pytest.mark.gpu
def test_pow2_kaldi_ragged_whole_batch(gpu, oracle):
    cus = _cus()
    sr = 8000.0
    fb, cfg, oc = _fbank(gpu, oracle, sr)
    fl, fs, nm = cfg.frame_length_samples(), cfg.frame_shift_samples(), fb.num_mel_bins
    lens, frames = ragged_batch(256, fl, fs, fl + 120 * fs, cus, 23)
    total = sum(frames)
    assert total >= 2 * s_max(256, cus) + 1 and trips_ok(total, 256, cus), (total, s_max(256, cus))
    assert frames == [fb.num_frames(n) for n in lens]
    base = _noise(len(lens), max(lens), 1400000)
    clips = [b[:n] for b, n in zip(base, lens)]
    want = _once(("kaldi-ragged", cus), lambda: _pmap(lambda x: oracle.fbank_compute(x, oc), clips))
    got = run_ragged(gpu, fb, np.concatenate(clips), lens, frames, nm)
    worst = _compare(got, want, TOL, "kaldi 8k ragged")
    print(f"\nWHOLE-BATCH generic/pow2 kaldi-8k-ragged: clips={len(lens)} frames={total} s_max={s_max(256, cus)} worst={worst:.3e}")
    fb.close()


# ---- 3. pow2_frame_kernel, NeMo flavour --------------------------------------------------------------------------------------------

# a geometry off the fused kernel (test_nemo_frontend_any_validated_geometry); 163 valid frames, 176 = 16 x 11 columns: the walk's
# units_per_clip is the padded width, and 11 divides no stride
NEMO_KW = dict(n_fft=1024, win_length=800, hop_length=256, pad_to=16, preemphasis=0.97)
NEMO_VALID, NEMO_COLS = 163, 176


@pytest.mark.gpu
@pytest.mark.parametrize("norm", [False, True], ids=["rows", "normalised"])
def test_pow2_nemo_whole_batch(gpu, oracle, norm):
    cus = _cus()
    kw = dict(NEMO_KW, normalize_per_feature=norm)
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    cfg = oracle.blm_default_config(**kw)
    fft, hop, nm = kw["n_fft"], kw["hop_length"], fe.config.n_mels
    n = (NEMO_VALID - 1) * hop + 100
    assert fe.num_frames(n) == NEMO_VALID and fe.padded_frames(n) == NEMO_COLS
    n_clips, f, upc, dups = pow2_batch("short", fft, cus, NEMO_VALID, NEMO_COLS)
    facts = check_recipe(n_clips, upc, dups, fft, cus)
    clips = with_copies(_noise(n_clips, n, 1500000 + 50000 * int(norm)), dups)
    want = _once(("nemo", norm, cus), lambda: _pmap(lambda x: oracle.blm_compute(x, cfg, True)[0], list(clips)))
    pcm, out = _upload(gpu, clips), Fence(gpu, n_clips * nm * upc)
    fe.compute_uniform_device(pcm.ptr, n, n, n_clips, out.ptr)
    fe.synchronize()
    bits = out.bits()
    pcm.free()
    _no_sentinel(bits, "nemo")
    got = bits.view(np.float32).reshape(n_clips, nm, upc)
    check_padding(got[:, :, f:], np.stack([w[:, f:] for w in want]), f"nemo norm={norm}")
    worst = compare_all(list(got), want, TOL, f"nemo norm={norm}")
    check_copies(got, dups, f"nemo norm={norm}")
    print(f"\nWHOLE-BATCH generic/pow2 nemo-1024-norm{int(norm)}: clips={n_clips} frames={n_clips * f} columns={n_clips * upc} worst={worst:.3e} {facts}")
    fe.close()


# ---- 4. generic_frame_kernel, Whisper flavour --------------------------------------------------------------------------------------

G300, G441 = (300, 100, SR, 40), (441, 160, SR, 64)
GENERIC_CASES = [(t, geo, kind) for t, geo in (("mixed", G300), ("direct", G441)) for kind in ("cap", "cap+1", "past")]


@pytest.mark.gpu
@pytest.mark.parametrize("case", GENERIC_CASES, ids=lambda c: f"{c[0]}-{c[2]}")
def test_generic_frame_kernel_whole_batch(gpu, oracle, case):
    """8 x CUs frames (one trip), 8 x CUs + 1 (one frame into the second), about 2.3 x 8 x CUs in clips of 37 (three trips, their
    boundaries inside clips): the mixed-radix transform of n_fft 300 and the direct DFT of the odd n_fft 441"""
    transform, geo, kind = case
    cus = _cus()
    fft, hop, sr, nm = geo
    n_clips, frames = generic_batch(kind, cus)
    check_generic_batch(kind, n_clips * frames, cus)
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    assert m.plain_kernel_name() == GENERIC
    clips = _noise(n_clips, fft + (frames - 1) * hop, 1600000 + 100000 * GENERIC_CASES.index(case))
    want = _once(("generic", transform, kind, cus), lambda: mel_oracle(oracle, clips, geo))
    got = run_uniform(gpu, m, clips, nm)
    worst = compare_all(got, want, F64_TOL, f"generic {transform} {kind}")
    print(f"\nWHOLE-BATCH generic/pow2 generic-{transform}-{kind}: n_fft={fft} clips={n_clips} frames={n_clips * frames} cap={8 * cus} worst={worst:.3e}")
    m.close()


@pytest.mark.gpu
def test_generic_frame_kernel_layout_whole_batch(gpu, oracle):
    """clips of 37 frames in a padded layout 78 columns wide, about 2.3 trips: zero columns written on the second and third"""
    cus = _cus()
    fft, hop, sr, nm = G300
    f, width = 37, 78
    n_clips = generic_layout_batch(cus, width)
    assert 2 * 8 * cus < n_clips * width < 3 * 8 * cus and (8 * cus) % width != 0
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    assert m.plain_kernel_name() == GENERIC
    n = fft + (f - 1) * hop
    assert m.interleaved_width(n, f + 41) == width
    clips = _noise(n_clips, n, 2300000)
    want = _once(("generic-layout", cus), lambda: mel_oracle(oracle, clips, G300))
    got = run_interleaved(gpu, m, clips, nm, True, f + 41)
    worst = compare_all(got, want, F64_TOL, "generic mixed padded")
    print(f"\nWHOLE-BATCH generic/pow2 generic-mixed-padded: clips={n_clips} frames={n_clips * f} columns={n_clips * width} cap={8 * cus} worst={worst:.3e}")
    m.close()


# ---- CPU: the recipes, the failing direction of the checks, the table against the source ----------------------------------------

def test_recipes_take_three_trips_whatever_the_waves_per_workgroup():
    """CU counts 64, 228, 256, 304, every waves per workgroup 1 .. kMaxWaves: each pow2 batch of the matrix takes at least three trips
    with a partial last one, the short shapes step by no whole number of clips, the copies start past the second trip; the generic
    kernel's cap, cap + 1 and 2.3 x cap batches are one, two and three trips"""
    for cus in CU_COUNTS:
        batches = [(fft, pow2_batch(shape, fft, cus, frames, frames + 41 if entry != "uniform" else None))
                   for _, (fft, _, _, _), shape, entry, frames, _ in WHISPER_CASES]
        batches += [(fft, pow2_batch("short", fft, cus, frames)) for fft, frames, _ in KALDI.values()]
        batches.append((NEMO_KW["n_fft"], pow2_batch("short", NEMO_KW["n_fft"], cus, NEMO_VALID, NEMO_COLS)))
        for fft, (n_clips, f, upc, dups) in batches:
            _, lf, fw, max_waves = POW2_SHAPE[fft]
            facts = check_recipe(n_clips, upc, dups, fft, cus)
            assert f <= upc and facts["trips_at_max_waves"] >= 3
            for w in range(1, max_waves + 1):
                stride = cus * w * fw
                groups = -(-n_clips * upc // (w * fw))
                assert min(groups, cus) == cus                       # launch_pow2: the grid is the CU count
                trips = -(-n_clips * upc // stride)
                assert trips >= 3 and n_clips * upc % stride != 0
                if upc > 1 and n_clips > 3:
                    assert stride % upc != 0
                for d in dups:
                    assert d * upc // stride >= 2                     # the copy's first frame: the third trip or later
            if n_clips == 3:                                         # long: the clips are shorter than a trip at the most waves
                assert 0.85 * s_max(fft, cus) <= f < s_max(fft, cus)
        for fft, frame_len, hop, n_max, seed in ((256, 256, 64, 256 + 150 * 64, 21), (256, 200, 80, 200 + 120 * 80, 23)):
            lens, frames = ragged_batch(fft, frame_len, hop, n_max, cus, seed)
            assert sum(frames) >= 2 * s_max(fft, cus) + 1 and len(lens) == len(frames) and min(lens) == 0
        cap = 8 * cus
        for kind, trips in (("cap", 1), ("cap+1", 2), ("past", 3)):
            n_clips, frames = generic_batch(kind, cus)
            check_generic_batch(kind, n_clips * frames, cus)
            assert -(-n_clips * frames // cap) == trips
        assert -(-generic_layout_batch(cus, 78) * 78 // cap) == 3
    assert s_max(128, 256) == 16384 and s_max(2048, 256) == 1536 and min_units(128, 256) == 40963 and min_units(2048, 256) == 3843
    seeds = [c[5] for c in WHISPER_CASES] + [v[2] for v in KALDI.values()]
    assert len(set(seeds)) == len(seeds)                             # every content distinct


def test_the_new_checks_fail_on_doctored_arrays():
    """a row shifted by one clip fails the comparison, a copy that differs in one bit fails the position check, a padding value that is
    not 0.0 fails the padding check -- and the undoctored arrays pass all three"""
    rng = np.random.default_rng(5)
    want = [rng.uniform(-1.0, 1.5, (37, 20)).astype(np.float32) for _ in range(12)]
    got = [w.copy() for w in want]
    assert compare_all(got, want, F64_TOL, "identical") == 0.0
    with pytest.raises(AssertionError, match="diff"):
        compare_all(got[1:] + got[:1], want, F64_TOL, "shifted by one clip")
    with pytest.raises(AssertionError, match="diff"):                # one frame of one clip taken from the clip before
        compare_all([g if c != 7 else np.vstack([g[:36], got[6][36:]]) for c, g in enumerate(got)], want, F64_TOL, "one frame of another clip")
    nan = [g.copy() for g in got]
    nan[3][5, 2] = np.nan
    with pytest.raises(AssertionError, match="diff"):
        compare_all(nan, want, F64_TOL, "a NaN")

    dups = (9, 10, 11)
    for k, d in enumerate(dups):
        got[d] = got[k].copy()
    check_copies(got, dups, "copies")
    check_copies([g.T for g in got], dups, "copies, transposed views")
    one_bit = [g.copy() for g in got]
    one_bit[10].view(np.uint32)[36, 19] ^= np.uint32(1)
    assert np.abs(one_bit[10] - got[10]).max() < 2e-7                # far below any tolerance
    with pytest.raises(AssertionError, match="position"):
        check_copies(one_bit, dups, "one bit")
    zero_sign = [g.copy() for g in got]
    zero_sign[0][0, 0], zero_sign[9][0, 0] = 0.0, -0.0
    with pytest.raises(AssertionError, match="position"):
        check_copies(zero_sign, dups, "the sign of a zero")

    pad = np.zeros((4, 80, 13), np.float32)
    check_padding(pad, np.zeros_like(pad), "zeros")
    for bad in (np.float32(1e-30), np.float32(np.nan), np.float32(SENTINEL.view(np.float32))):
        doctored = pad.copy()
        doctored[3, 79, 12] = bad
        with pytest.raises(AssertionError, match="padding"):
            check_padding(doctored, np.zeros_like(pad), "one value")
    with pytest.raises(AssertionError, match="padding"):             # agreeing with an oracle whose padding is not 0.0 is not enough
        check_padding(np.ones_like(pad), np.ones_like(pad), "ones")


def _define(src, name):
    m = re.search(r"#ifndef %s\n#define %s (\d+)" % (name, name), src)
    assert m, name
    return int(m.group(1))


def test_pow2_shape_table_is_the_sources():
    """POW2_SHAPE restates Pow2Shape's LF / FW / kMaxWaves (pow2_wave.hpp) and launch_pow2's stride (pow2.hip, generic_kernels.hpp): the
    formulas are matched as text and the knobs' defaults are read from the header, so a change there fails here"""
    csrc = os.path.join(ROOT, "mel_spec_amd", "csrc")
    wave = open(os.path.join(csrc, "pow2_wave.hpp")).read()
    for line in ("static constexpr int LF = M >= 512 ? 64 : M / 8;", "static constexpr int FW = 64 / LF;",
                 "static constexpr bool kHalves = MS_POW2_HALVES && M >= 1024;",
                 "static constexpr int kMaxWaves = M >= 1024 ? (kHalves ? MS_POW2_MAXWH : MS_POW2_MAXW16) : MS_POW2_MAXW;"):
        assert line in wave, line
    maxw, maxwh, maxw16, halves = (_define(wave, k) for k in ("MS_POW2_MAXW", "MS_POW2_MAXWH", "MS_POW2_MAXW16", "MS_POW2_HALVES"))
    launch = open(os.path.join(csrc, "pow2.hip")).read()
    assert "const unsigned grid = grid_for(groups, cus, 1);" in launch and "dim3(waves * 64)" in launch
    assert "MS_POW2_CASE(7, 6) MS_POW2_CASE(8, 7) MS_POW2_CASE(9, 8) MS_POW2_CASE(10, 9) MS_POW2_CASE(11, 10)" in launch
    assert "const unsigned grid = grid_for(desc.n_units, cus, 8);" in launch                  # generic_frame_kernel's cap
    kernels = open(os.path.join(csrc, "generic_kernels.hpp")).read()
    assert "const uint64_t stride = (uint64_t)gridDim.x * n_waves * FW;" in kernels
    assert "for (uint64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {" in kernels
    assert sorted(POW2_SHAPE) == [128, 256, 512, 1024, 2048]
    for n_fft, (logm, lf, fw, max_waves) in POW2_SHAPE.items():
        M = n_fft // 2
        assert 1 << logm == M and 1 << (logm + 1) == n_fft
        assert lf == (64 if M >= 512 else M // 8) and fw == 64 // lf
        assert max_waves == ((maxwh if halves else maxw16) if M >= 1024 else maxw)
        assert f"pow2_frame_kernel<{logm}, kFlavorWhisper> (n_fft = {n_fft}" in POW2[logm]
