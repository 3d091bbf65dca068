"""The f32 kernels gated on their mean error and on their per-band and per-slot bias, not only on their largest error.

Every other comparison of an f32 kernel with the oracle bounds the LARGEST difference (1e-4 in AUTO, 6e-4 in F32 mode, max(1e-4, 4 x the
reference's own f32 error) for NeMo F32): gates sized for the f32 FFT's worst case, a line over a quiet floor.  On input without
cancellation the kernels sit thousands of times below them, so a wrong table entry, window tap, twiddle digit or slot weight that moves
a band's energy by 1e-3 relative (1e-4 of output) passes all of them.  The signed mean error of a band over a few thousand frames sees
such a shift two to three orders of magnitude earlier.

Yardstick: an independent honest f32 evaluation of the same definition on the same clips, computed inside each test (no constant is
committed) -- whisper_f32 below (numpy float32 throughout, scipy's float32 rfft) for the Whisper flavours, the oracle's literal f32
restatement of the reference (blm_compute(x, cfg, False)) for NeMo.  A row asserts, with e = got - the f64 oracle over every valid frame,

    mean|e|        <= MARGIN x the yardstick's
    band bias      <= MARGIN x max(the yardstick's band bias, 3 x standard error)       max over bands of |mean over frames of e[:, b]|
    slot bias      <= MARGIN x max(the yardstick's slot bias, 3 x standard error)       the same per frame index mod frames-per-unit
    max|e|         <= the suite's gate of that mode, unchanged

with the yardstick's per-band standard error, which is asserted to be <= 0.25 x the yardstick's band bias, so the bias gate measures
bias and not sample size.  MARGIN = 4: the kernels' arithmetic run on the host (tests/emu) sits at 1.0 - 2.5 x the yardstick, the device at
2.4 - 2.9 x (profiles/f32_stats.txt); the smallest perturbation of the CPU test below sits at ~6 x.  The NeMo rows' bias gates on the
device: NEMO_BIAS_MARGIN.

Input: hash noise and Gaussian noise at 0.1 -- no speech, no tones (cancellation is what the max gates and the guard tests are for, and
it would drown the statistic).  Whisper values at or within 1e-3 of the per-frame clamp are left out of the means; on this input there
are none (asserted <= 1 %, and == 0 for the oracle).  With normalize_per_feature the statistic belongs on the raw twin's rows (the
normaliser is gated in tests/test_gpu_parity.py and tests/test_blm_split*.py): every NeMo row here runs un-normalised."""
import ctypes as C
import functools
import os
import subprocess
from typing import NamedTuple

import numpy as np
import pytest
import scipy.fft
import torch   # before libmelspec_hip.so is loaded (tests/test_whole_batch.py)  # noqa: F401

from conftest import ROOT
from test_f32_512 import _nemo_gate
from test_whole_batch import (F32_TOL, F64_TOL, FAMILIES, G40, G60, G64, G80, G84, G100, G128, G512, SR, THREADS, TOL, Fence, _auto_pass,
                              _no_sentinel, _noise, _pmap, _upload, run_interleaved, run_ragged, run_uniform)

MARGIN = 4.0            # see the module docstring; never above 16, where an error of (1 + 1e-5) on a whole band stops being seen
# The bias gates of the NeMo F32 rows on the device.  Measured at MARGIN (profiles/f32_stats.txt): mean x 2.4, band bias x 3.8 - 4.0, slot
# bias x 5.0 - 5.4 on the 80-mel configurations -- the same offset of -2.4e-7 in every band and slot, so neither a table nor the lane
# algebra.  It is the log: this frontend's output is ln(E + g) = v_log_f32(E + g) * ln2f (fast_ln, fbank_wave.hpp), and v_log_f32 is
# within its 1 ulp but not centred: measured on the device over this output's range, v_log_f32 - log2 has a mean of -0.44 .. -0.47 ulp
# (worst 1.00), which is -2.0e-7 .. -3.0e-7 of ln, where log2f * ln2f on the host has -1.2e-8.  The same kernel source in f32 on the
# host (emu_blm_wave_f32, CPU test below) sits at x 1.5.  The Whisper rows carry the log too, divided by 4 ln 10 (-1.7e-8 .. -2.5e-8 of
# output): inside MARGIN (x 2.1 on the slot bias).  8 = 1.5 x the largest measured ratio (at most 2 x; at most 16): a band x (1 + 1e-5)
# moves this output by 1e-5, 18 x the gate.  The mean gate, and Parakeet's rows (whose floor, 3 x se, is above the offset), stay at MARGIN.
NEMO_BIAS_MARGIN = 8.0
CLIP_N = 16000 + 37
N_CLIPS = 40            # 30 of hash noise, 10 Gaussian: 3 920 frames at 400 / 160, 4 040 columns on the centred NeMo frontend
G512_128 = (512, 160, SR, 128)


# ---- 1. the yardstick ---------------------------------------------------------------------------------------------------------------

def whisper_f32(x, n_fft, hop, n_mels, sr, *, window=None, bank=None, dtype=np.float32, energies=False):
    """compute_mel_spectrogram_cpu in float32 throughout: frames x Hann, scipy's float32 rfft, re^2 + im^2, the product with the
    float32 mel bank, log10(max(., 1e-10)), the max - 8 clamp of the frame (norm_mel_slice: the maximum is the frame's), (v + 4) / 4.
    window / bank (f64, rounded here): a perturbed table in place of the oracle's, for the CPU test of the gates.  dtype: the type
    everything runs in (np.float64: the unrounded evaluation of tests/test_f64_statistics.py); energies: -> (out, the mel energies)"""
    from oracle import oracle as O
    f32 = np.dtype(dtype).type
    x = np.ascontiguousarray(x, f32)
    nf = 0 if x.shape[0] < n_fft else (x.shape[0] - n_fft) // hop + 1
    if nf == 0:
        return (np.zeros((0, n_mels), f32),) * 2 if energies else np.zeros((0, n_mels), f32)
    w = np.asarray(O.hann_window(n_fft) if window is None else window).astype(f32)
    fb = np.asarray(O.mel_filterbank(sr, n_fft, n_mels) if bank is None else bank).astype(f32)
    frames = np.lib.stride_tricks.sliding_window_view(x, n_fft)[::hop][:nf] * w
    assert frames.dtype == f32
    z = scipy.fft.rfft(frames, axis=1)
    assert z.dtype == (np.complex64 if f32 is np.float32 else np.complex128)
    p = z.real * z.real + z.imag * z.imag
    e = p @ fb.T
    v = np.log10(np.maximum(e, f32(1e-10)))
    v = np.maximum(v, v.max(axis=1, keepdims=True) - f32(8.0))
    out = (v + f32(4.0)) / f32(4.0)
    assert out.dtype == f32 and out.shape == (nf, n_mels)
    return (out, e) if energies else out


# ---- 2. the statistic ---------------------------------------------------------------------------------------------------------------

class Stats(NamedTuple):
    max: float      # max|e|, every value
    mean: float     # mean|e|
    band: float     # the largest |mean over frames of e[:, b]|
    slot: float     # the largest |mean of e over the frames with index = s mod fpu|
    se: float       # the largest per-band standard error sd_b / sqrt(N_b)
    off: float      # the signed mean of e: what every band and slot has in common
    frames: int
    share: float    # of the values left out of the means (Whisper: at or within 1e-3 of the frame's clamp)


def err_stats(got, want, fpu, clamp=True, bands=None):
    """got / want: per clip [frames, mels] (want: the f64 oracle); e = got - want in float64 over every frame of every clip; the slot of a
    frame is its index in the clip mod fpu.  clamp: a Whisper output -- the values the frame's max - 8 clamp made (in units of the output:
    want <= the frame's maximum - 2) or nearly made (within 1e-3) are left out of the means.  bands: a list that receives the signed
    mean of e per band (Stats.band is the largest of them in magnitude)."""
    pairs = [(np.asarray(g), np.asarray(w)) for g, w in zip(got, want)]
    for g, w in pairs:
        assert g.shape == w.shape and g.ndim == 2, (g.shape, w.shape)
    pairs = [(g, w) for g, w in pairs if w.shape[0]]
    e = np.concatenate([g.astype(np.float64) - w.astype(np.float64) for g, w in pairs])
    w = np.concatenate([w.astype(np.float64) for _, w in pairs])
    slot = np.concatenate([np.arange(w.shape[0]) % fpu for _, w in pairs])
    keep = w > w.max(axis=1, keepdims=True) - 2.0 + 1e-3 if clamp else np.ones(w.shape, bool)
    n_b = keep.sum(axis=0)
    assert n_b.min() >= 2, "a band without values outside the clamp"
    mean_b = np.where(keep, e, 0.0).sum(axis=0) / n_b
    var_b = np.where(keep, (e - mean_b) ** 2, 0.0).sum(axis=0) / (n_b - 1)
    if bands is not None:
        bands.append(mean_b)
    slots = [float(np.abs(e[slot == s][keep[slot == s]].mean())) for s in range(fpu) if keep[slot == s].any()]
    return Stats(float(np.abs(e).max()), float(np.abs(e[keep]).mean()), float(np.abs(mean_b).max()), max(slots),
                 float(np.sqrt(var_b / n_b).max()), float(e[keep].mean()), int(e.shape[0]), float(1.0 - keep.mean()))


def gate_failures(dev, yard, max_tol, margin=MARGIN, must_see=None, bias_margin=None):
    """the names of the gates `dev` misses against the yardstick's statistics (NaN misses every one).  must_see: a row whose input cannot
    meet the sample-size condition (SAMPLE_LIMITED) -- the bias gate is at most half this shift of a band instead"""
    floor_b, floor_s = max(yard.band, 3.0 * yard.se), max(yard.slot, 3.0 * yard.se)
    bias_margin = margin if bias_margin is None else bias_margin
    sized = yard.se <= 0.25 * yard.band if must_see is None else bias_margin * floor_b <= 0.5 * must_see
    checks = (("clamp share", dev.share <= 0.01), ("sample size", sized),
              ("mean", dev.mean <= margin * yard.mean), ("band bias", dev.band <= bias_margin * floor_b),
              ("slot bias", dev.slot <= bias_margin * floor_s), ("max", dev.max <= max_tol))
    return [name for name, ok in checks if not ok]


def report(rid, dev, yard, tag="F32-STATS", tail=""):
    floor_b, floor_s = max(yard.band, 3.0 * yard.se), max(yard.slot, 3.0 * yard.se)
    ratio = max(dev.mean / yard.mean, dev.band / floor_b, dev.slot / floor_s)
    print(f"\n{tag} {rid} frames={dev.frames} max={dev.max:.2e} mean={dev.mean:.2e} bias={dev.band:.2e} slot={dev.slot:.2e} "
          f"se={dev.se:.1e} off={dev.off:+.2e} | yardstick max={yard.max:.2e} mean={yard.mean:.2e} bias={yard.band:.2e} slot={yard.slot:.2e} se={yard.se:.1e} off={yard.off:+.2e} | "
          f"mean x{dev.mean / yard.mean:.2f} bias x{dev.band / floor_b:.2f} slot x{dev.slot / floor_s:.2f} ratio={ratio:.2f}{tail}")


def check(rid, dev, yard, max_tol, must_see=None, bias_margin=None):
    report(rid, dev, yard)
    bad = gate_failures(dev, yard, max_tol, must_see=must_see, bias_margin=bias_margin)
    assert not bad, f"{rid}: misses {bad}: {dev} against the yardstick's {yard} (margin {MARGIN}, on the bias {bias_margin or MARGIN}, max gate {max_tol:.1e})"


# ---- 3. inputs and references, computed once ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _clips(n_clips=N_CLIPS):
    """three clips of hash noise to one of Gaussian noise at 0.1, read-only"""
    rng = np.random.default_rng(20)
    gauss = (0.1 * rng.standard_normal((n_clips // 4, CLIP_N))).astype(np.float32)
    a = np.concatenate([_noise(n_clips - n_clips // 4, CLIP_N, 11000), gauss])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _whisper_ref(geo, n_clips=N_CLIPS):
    """-> (clips, the f64 oracle, the yardstick), [clips, frames, mels] each"""
    from oracle import oracle as O
    fft, hop, sr, nm = geo
    clips = _clips(n_clips)
    want = O.compute_mel_batch(clips, fft, hop, nm, sr, THREADS)
    yard = np.stack(_pmap(lambda x: whisper_f32(x, fft, hop, nm, sr), list(clips)))
    for a in (want, yard):
        a.setflags(write=False)
    return clips, want, yard


def _frames_of(n, fft, hop):
    return 0 if n < fft else (n - fft) // hop + 1


def ragged_lens(fft, hop, fpu, n_clips=N_CLIPS):
    """most clips whole; an empty one, sub-frame, exactly one frame (with and without spare samples), fpu k +- 1 frames"""
    at = lambda f: fft + (f - 1) * hop
    lens = [CLIP_N] * n_clips
    for i, v in enumerate((0, fft - 1, fft, fft + hop - 1, at(2 * fpu - 1), at(2 * fpu + 1), at(7 * fpu - 1) + 3, at(7 * fpu + 1), at(fpu))):
        lens[(4 * i + 1) % n_clips] = v
    return lens


NEMO_CFGS = {
    "default": dict(),
    "parakeet": dict(n_mels=128, preemphasis=0.97, log_zero_guard=2.0 ** -24),
    "nocenter": dict(center=False),
    "pad16": dict(pad_to=16),
}
NEMO_FPU = FAMILIES["f512_32"][2]
NEMO_EDGE_LENS = (1, 399, 400, 401, 511, 512, 559, 560)       # tests/test_blm_io_dtypes.py's, around win_length = 400 and n_fft = 512
NEMO_EDGE_FRAMES = (4 * 3 - 1, 4 * 3 + 1, 4 * 5)              # fpu k +- 1, fpu k
# Parakeet's config on broadband noise: pre-emphasis 0.97 leaves the lower bands of the 128-mel bank ~30 dB under the rest and the 2^-24
# guard does not cover them, so ANY f32 FFT's error there has a heavy tail -- the reference's literal f32: max|e| 2.7e-4 against a mean
# of 6.7e-7, a standard deviation of 1.3e-5 in band 0, the largest per-band standard error 2.1e-7 on 4 040 frames where the largest
# band bias that is not noise is 8e-8 (band 61, se 2e-9; 32 320 frames: se 6.5e-8).  se <= 0.25 x the band bias would take ~3e5 frames:
# minutes of oracle.  The bias gate's floor is 3 x the standard error there, as the gate's formula has it; what the test asserts of the
# sample in its place is that the gate still sees, twice over, what the margin's cap of 16 is derived from: all weights of one band
# x (1 + 1e-5), a shift of 1e-5 of this frontend's natural-log output.
SAMPLE_LIMITED = {"parakeet": 1e-5}


def nemo_lens(center, n_clips=N_CLIPS):
    at = (lambda f: (f - 1) * 160) if center else (lambda f: 512 + (f - 1) * 160)
    lens = [CLIP_N] * n_clips
    for i, v in enumerate(NEMO_EDGE_LENS + tuple(at(f) for f in NEMO_EDGE_FRAMES)):
        lens[(3 * i + 1) % n_clips] = v
    return lens


def _nemo_stats(name, imgs, want, valid):
    return err_stats(_rows(imgs, valid), _rows(want, valid), NEMO_FPU, clamp=False)


@functools.lru_cache(maxsize=None)
def _nemo_ref(name, ragged):
    """-> (clips, their lengths, per clip: the f64 evaluation [mels, cols], valid columns, the reference's literal f32 [mels, cols])"""
    from oracle import oracle as O
    cfg = O.blm_default_config(**{k: (int(v) if isinstance(v, bool) else v) for k, v in NEMO_CFGS[name].items()})
    lens = nemo_lens(NEMO_CFGS[name].get("center", True)) if ragged else [CLIP_N] * N_CLIPS
    xs = [np.ascontiguousarray(c[:n]) for c, n in zip(_clips(), lens)]
    both = _pmap(lambda x: (O.blm_compute(x, cfg, True), O.blm_compute(x, cfg, False)[0]), xs)
    return xs, lens, [b[0][0] for b in both], [b[0][1] for b in both], [b[1] for b in both]


def _rows(imgs, valid):
    """[mels, cols] images -> [valid frames, mels]: the pad columns are left out"""
    return [np.ascontiguousarray(a[:, :v].T) for a, v in zip(imgs, valid)]


# ---- 5. CPU: the gates see a subtly wrong evaluation, hold for the kernels' arithmetic on the host, and the inputs are what they claim --

def _perturbed(kind, nm=80):
    from oracle import oracle as O
    fft, hop, sr, _ = G80
    win, bank = O.hann_window(fft), O.mel_filterbank(sr, fft, nm)
    if kind == "one weight x (1 + 2e-4)":
        bank[3, int(np.argmax(bank[3]))] *= 1.0 + 2e-4
    elif kind == "one band x (1 + 1e-5)":
        bank[41] *= 1.0 + 1e-5
    elif kind == "Hann tap 57 x (1 + 1e-3)":
        win[57] *= 1.0 + 1e-3
    else:
        raise ValueError(kind)
    return np.stack([whisper_f32(x, fft, hop, nm, sr, window=win, bank=bank) for x in _clips()])


@pytest.mark.parametrize("kind,under_max", [("one weight x (1 + 2e-4)", True), ("one band x (1 + 1e-5)", True), ("Hann tap 57 x (1 + 1e-3)", None)])
def test_gates_are_red_on_a_subtly_wrong_evaluation(oracle, kind, under_max):
    """a wrong bank entry, a wrong band scale, a wrong window tap in the f32 evaluation: far inside the 1e-4 max gate of the suite (the
    first two: asserted), and red on the band bias"""
    _, want, yard = _whisper_ref(G80)
    y = err_stats(yard, want, 6)
    bad = err_stats(_perturbed(kind), want, 6)
    report(f"cpu-perturbed[{kind}]", bad, y)
    missed = gate_failures(bad, y, TOL)
    assert "band bias" in missed, (kind, bad, y)
    if under_max:
        assert "max" not in missed and bad.max <= TOL, (kind, bad)
    assert not gate_failures(y, y, TOL)


@pytest.fixture(scope="module")
def emu_lib():
    d = os.path.join(ROOT, "tests", "emu")
    subprocess.check_call(["make", "-C", d, "-s"])
    L = C.CDLL(os.path.join(d, "libmelspec_emu.so"))
    f32p = C.POINTER(C.c_float)
    for name in ("emu_whisper_six", "emu_whisper_wave"):
        getattr(L, name).restype = C.c_longlong
        getattr(L, name).argtypes = [f32p, C.c_longlong, C.c_int, C.c_int, C.c_double, C.c_int, f32p]
    L.emu_w512_wave.restype = C.c_longlong
    L.emu_w512_wave.argtypes = [f32p, C.c_longlong, C.c_int, C.c_int, C.c_double, f32p]
    L.emu_blm_wave_f32.restype = C.c_longlong
    L.emu_blm_wave_f32.argtypes = [f32p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, C.c_int, C.c_float, C.c_int, C.c_float,
                                   C.c_longlong, f32p]
    return L


EMU_ROWS = [("emu_whisper_six", G80, 6), ("emu_whisper_wave", G80, 5), ("emu_whisper_wave", G128, 5), ("emu_w512_wave", G512, 4),
            ("emu_w512_wave", G512_128, 4)]


@pytest.mark.parametrize("entry,geo,fpu", EMU_ROWS, ids=[f"{r[0]}-{r[1][3]}" for r in EMU_ROWS])
def test_gates_hold_for_the_kernels_arithmetic_on_the_host(oracle, emu_lib, entry, geo, fpu):
    """tests/emu runs the kernels' own phase functions lane by lane (compile-time slot lengths, as the library picks them for these banks;
    emu_w512_wave is the f64 instantiation of the 512-point kernel's source, the only one tests/emu has)"""
    fft, hop, sr, nm = geo
    clips, want, yard = _whisper_ref(geo)
    f32p = C.POINTER(C.c_float)

    def run(x):
        out = np.full((_frames_of(x.shape[0], fft, hop), nm), np.nan, np.float32)
        args = (x.ctypes.data_as(f32p), x.shape[0], hop, nm, sr) + ((1,) if fft == 400 else ()) + (out.ctypes.data_as(f32p),)
        assert getattr(emu_lib, entry)(*args) == out.shape[0]
        return out

    got = _pmap(run, [np.ascontiguousarray(x) for x in clips])
    check(f"cpu-{entry}-{nm}", err_stats(got, want, fpu), err_stats(yard, want, fpu), TOL)


@pytest.mark.parametrize("name", list(NEMO_CFGS))
def test_gates_hold_for_the_nemo_kernels_arithmetic_on_the_host(oracle, emu_lib, name):
    """the 512-point kernel's source instantiated in f32 and run lane by lane on the host, with the host's log2f: what the device adds to
    this is its own log (v_log_f32) and its contraction choices -- NEMO_MARGIN"""
    from oracle import oracle as O
    xs, lens, want, valid, lit = _nemo_ref(name, False)
    cfg = O.blm_default_config(**{k: (int(v) if isinstance(v, bool) else v) for k, v in NEMO_CFGS[name].items()})
    f32p = C.POINTER(C.c_float)

    def run(item):
        x, w, v = item
        out = np.full_like(w, np.nan)
        assert emu_lib.emu_blm_wave_f32(x.ctypes.data_as(f32p), x.shape[0], cfg.hop_length, cfg.n_mels, cfg.sample_rate, cfg.f_min, cfg.f_max, cfg.htk,
                                        cfg.norm, cfg.preemphasis, cfg.center, cfg.log_zero_guard, w.shape[1], out.ctypes.data_as(f32p)) == v
        return out

    got = _pmap(run, list(zip(xs, want, valid)))
    y = _nemo_stats(name, lit, want, valid)
    check(f"cpu-emu_blm_wave_f32-{name}", _nemo_stats(name, got, want, valid), y, max(1.5 * TOL, 4.0 * y.max),     # tests/test_whole_batch.py's gate of this mode
          must_see=SAMPLE_LIMITED.get(name))


@pytest.mark.parametrize("geo,fpu", [(G80, 6), (G64, 6), (G40, 6), (G128, 6), (G60, 6), (G84, 5), (G100, 5), (G512, 4), (G512_128, 4)],
                         ids=lambda v: f"{v[0]}-{v[3]}" if isinstance(v, tuple) else None)
def test_whisper_inputs_and_yardstick(oracle, geo, fpu):
    """the inputs are what the gates assume: nothing at the clamp (the oracle alone: exactly nothing), >= 2 000 frames per row, a
    standard error a quarter of the yardstick's band bias or less -- uniform and ragged; and the yardstick's own figures, printed"""
    fft, hop, sr, nm = geo
    clips, want, yard = _whisper_ref(geo)
    assert err_stats(want, want, fpu).share == 0.0
    frames = [_frames_of(n, fft, hop) for n in ragged_lens(fft, hop, fpu)]
    assert sorted(set(frames))[:2] == [0, 1] and {2 * fpu - 1, 2 * fpu + 1, 7 * fpu - 1, 7 * fpu + 1, fpu} <= set(frames)
    for what, w, y in (("uniform", want, yard), ("ragged", [a[:f] for a, f in zip(want, frames)], [a[:f] for a, f in zip(yard, frames)])):
        s = err_stats(y, w, fpu)
        report(f"cpu-yardstick-{fft}-{nm}-{what}", s, s)
        assert s.frames >= 2000 and s.share == 0.0
        assert not gate_failures(s, s, TOL), (what, s)


@pytest.mark.parametrize("name", list(NEMO_CFGS))
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_nemo_inputs_and_yardstick(oracle, name, ragged):
    xs, lens, want, valid, lit = _nemo_ref(name, ragged)
    assert all(w.shape == a.shape for w, a in zip(want, lit))
    if ragged:
        assert min(valid) <= 1 and set(NEMO_EDGE_FRAMES) <= set(valid)
    s = _nemo_stats(name, lit, want, valid)
    report(f"cpu-yardstick-nemo-{name}-{'ragged' if ragged else 'uniform'}", s, s)
    assert s.frames >= 2000
    assert not gate_failures(s, s, 1.0, must_see=SAMPLE_LIMITED.get(name)), s
    assert name in SAMPLE_LIMITED or "sample size" not in gate_failures(s, s, 1.0)


# ---- 6. GPU rows -------------------------------------------------------------------------------------------------------------------

W400 = {"six80": (G80, "six16"), "six64": (G64, "six12"), "six40": (G40, "six12"), "six128": (G128, "six12"), "sixrt": (G60, "six16"),
        "wave8": (G84, "wave"), "wave12": (G100, "wave")}
WHISPER_ROWS = [(f"{key}-{prec or 'auto'}-uniform", geo, fam, prec, "uniform") for key, (geo, fam) in W400.items() for prec in ("f32", None)]
WHISPER_ROWS += [(f"{key}-f32-{entry}", *W400[key], "f32", entry) for key in ("six80", "six128") for entry in ("ragged", "padded", "melmajor", "stream")]
WHISPER_ROWS += [(f"w512-{geo[3]}-f32-{entry}", geo, "f512_32", "f32", entry) for geo in (G512, G512_128) for entry in ("uniform", "melmajor")]


def _whisper_max_gate(prec):
    if prec == "f32":
        return F32_TOL
    return TOL if _auto_pass() else F64_TOL


def _stream_rows(gpu, m, clips, chunk):
    """one StreamBank, a stream per clip, pushed in chunks of `chunk` samples -> per stream, the rows of each push"""
    bank = gpu.StreamBank(m, clips.shape[0], chunk)
    ids = list(range(clips.shape[0]))
    got = [[] for _ in ids]
    for p in range(0, clips.shape[1], chunk):
        for s, r in zip(ids, bank.push(ids, [c[p:p + chunk] for c in clips])):
            got[s].append(np.array(r))
    bank.close()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("rid,geo,fam,prec,entry", WHISPER_ROWS, ids=[r[0] for r in WHISPER_ROWS])
def test_whisper_f32_statistics(gpu, oracle, rid, geo, fam, prec, entry):
    if prec is not None and not _auto_pass():
        pytest.skip("a row with an explicit precision runs once, in the default-mode pass")
    fft, hop, sr, nm = geo
    fpu = FAMILIES[fam][2]
    clips, want, yard = _whisper_ref(geo)
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    if prec is not None:
        m.set_precision(prec)
        assert m.precision == prec
    else:
        m.guard_last_count()
    if entry == "uniform":
        got = run_uniform(gpu, m, clips, nm)
    elif entry in ("padded", "melmajor"):
        got = run_interleaved(gpu, m, clips, nm, entry == "padded", want.shape[1] + 42)
    elif entry == "ragged":
        lens = ragged_lens(fft, hop, fpu)
        frames = [m.num_frames(n) for n in lens]
        assert frames == [_frames_of(n, fft, hop) for n in lens]
        got = run_ragged(gpu, m, np.concatenate([c[:n] for c, n in zip(clips, lens)]), lens, frames, nm)
        want, yard = [a[:f] for a, f in zip(want, frames)], [a[:f] for a, f in zip(yard, frames)]
    else:
        # the streaming frames are the batch frames of samples[off:], off = ceil(n_fft / hop) hop - n_fft (tests/test_stream.py): the
        # oracle's streaming loop, and the yardstick on the same alignment; a push's rows are a launch's clip (slots count from its first)
        off = -(-fft // hop) * hop - fft
        pushes = _stream_rows(gpu, m, clips, 4000)
        got, want_s, yard_s = [], [], []
        for x, per_push in zip(clips, pushes):
            w = oracle.stream_mel(x, fft, hop, nm, sr)
            y = whisper_f32(x[off:], fft, hop, nm, sr)[:w.shape[0]]
            assert sum(r.shape[0] for r in per_push) == w.shape[0] == y.shape[0]
            cuts = np.cumsum([0] + [r.shape[0] for r in per_push])
            got += per_push
            want_s += [w[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
            yard_s += [y[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        want, yard = want_s, yard_s
    if prec is None and _auto_pass() and nm in (80, 128):
        assert m.guard_last_count() == 0      # noise queues nothing (tests/test_gpu_parity.py): the row is the f32 kernel alone
    m.close()
    check(rid, err_stats(got, want, fpu), err_stats(yard, want, fpu), _whisper_max_gate(prec))


@pytest.mark.gpu
def test_whisper512_auto_statistics_on_a_voting_batch(gpu, oracle):
    """more than 24 576 frames: AUTO votes, the batch is light, and the f32 kernel serves it (the f64-initial pass: the f64 kernel)"""
    n_clips = 252
    clips, want, yard = _whisper_ref(G512, n_clips)
    assert want.shape[0] * want.shape[1] > 24576
    m = gpu.HipMelSpectrogram(*G512)
    got = run_uniform(gpu, m, clips, 80)
    if _auto_pass():
        assert m.precision == "auto" and not m.auto_state()[0]
    m.close()
    check("w512-80-auto-uniform", err_stats(got, want, 4), err_stats(yard, want, 4), _whisper_max_gate(None))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NEMO_CFGS))
@pytest.mark.parametrize("ragged", [False, True], ids=["uniform", "ragged"])
def test_nemo_f32_statistics(gpu, oracle, name, ragged):
    if not _auto_pass():
        pytest.skip("a row with an explicit precision runs once, in the default-mode pass")
    kw = NEMO_CFGS[name]
    nm = kw.get("n_mels", 80)
    xs, lens, want, valid, lit = _nemo_ref(name, ragged)
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    fe.set_precision("f32")
    assert fe.precision == "f32"
    cols = [fe.padded_frames(n) for n in lens]
    assert [w.shape for w in want] == [(nm, c) for c in cols] and valid == [fe.num_frames(n) for n in lens]
    pcm, out = _upload(gpu, np.concatenate(xs)), Fence(gpu, nm * sum(cols))
    if ragged:
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        fe.compute_ragged_device(pcm.ptr, offs, np.array(lens, np.uint64), out.ptr)
    else:
        fe.compute_uniform_device(pcm.ptr, CLIP_N, CLIP_N, len(xs), out.ptr)
    fe.synchronize()
    bits = out.bits()
    pcm.free()
    fe.close()
    if not ragged:
        _no_sentinel(bits, "nemo")
    got, cur = [], 0
    for c in cols:
        got.append(bits[cur:cur + nm * c].view(np.float32).reshape(nm, c))
        cur += nm * c
    # the largest difference: the suite's gate of this mode (tests/test_f32_512.py), per clip
    for g, w, a, v in zip(got, want, lit, valid):
        if v:
            d, gate = _nemo_gate(g[:, :v], w[:, :v].astype(np.float64), a[:, :v])
            assert d <= gate, (name, d, gate)
    check(f"nemo-{name}-{'ragged' if ragged else 'uniform'}", _nemo_stats(name, got, want, valid), _nemo_stats(name, lit, want, valid), 1.0,
          must_see=SAMPLE_LIMITED.get(name), bias_margin=MARGIN if name in SAMPLE_LIMITED else NEMO_BIAS_MARGIN)
