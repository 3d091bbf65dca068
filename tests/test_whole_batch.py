"""Whole GPU batches, every frame of every clip against the oracle, in fenced output buffers.

The parity tests elsewhere compare a sample of each batch on buffers whose old contents are plausible outputs.  Here every device
entry point writes into the middle of an allocation filled with a NaN sentinel (payload 0x7fc0dead, which no kernel computes), with a
guard band on each side, and the whole output is checked: the guard bands are intact, no sentinel is left where a frame belongs, layout
padding is exactly 0.0, the gaps between ragged outputs still hold the sentinel -- and every frame agrees with the oracle.

Batch sizes are chosen at the edges of the run-per-wave partition of the plain kernels (ClipRun::init, kernels_common.hpp: each of
grid x waves waves takes a contiguous run of ceil(units / (grid x waves)) units; grid_for_xcd, host_common.hpp): fewer units than
waves, exactly grid x waves units, k x grid x waves + 1 units, and runs whose boundaries fall inside clips.  The CPU test at the end
keeps the matrix in step with melspec_plain_kernel_name (ctx_route.hpp, fused512_route.hpp, pow2.hip): every name it can return has a row here."""
import os
import re
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py): the device properties come from here

from conftest import ROOT

SR = 16000.0
TOL = 1e-4
F64_TOL = 2e-6        # the f64 kernels' gate (tests/test_gpu_parity.py, tests/test_auto_512.py)
F32_TOL = 6e-4        # MELSPEC_PRECISION_F32 of the n_fft = 400 kernels (tests/test_gpu_parity.py, tests/test_f32_512.py)
SENTINEL = np.uint32(0x7FC0DEAD)
GUARD = 2048          # floats of guard band on each side of an output: 8 KiB
THREADS = 16


def _auto_pass():
    return os.environ.get("MELSPEC_PRECISE", "")[:1] == ""


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _tone_over_floor(n, level_db, f, seed):
    t = np.arange(n) / SR
    rng = np.random.default_rng(seed)
    return (0.9 * np.sin(2 * np.pi * f * t) + 10 ** (level_db / 20) * rng.standard_normal(n)).astype(np.float32)


# ---- the partition of the plain kernels -------------------------------------------------------------------------------------------

# waves per workgroup, workgroups per CU, frames per unit of the kernel a plain batch runs on (the launchers in whisper400.hip and
# fbank512.hip; kSixWaves, kSixWideWaves, kWaveWaves, kPreciseWaves, kSix64Waves, kFused512F32Waves; kSixFrames, kFPW, kFbFPW)
FAMILIES = {
    "six16": (16, 1, 6),      # whisper400_six_runs_kernel<9, .>
    "six12": (12, 1, 6),      # whisper400_six_wide_runs_kernel<9 | 15, .>
    "wave": (8, 4, 5),        # whisper400_wave_runs_kernel
    "precise": (8, 1, 5),     # whisper400_precise_kernel
    "six64": (12, 1, 6),      # whisper400_six64_kernel
    "f512_32": (12, 1, 4),    # fbank512_wave_kernel<float, 12>, w512_auto_kernel<float, 12>
    "f512_64": (8, 1, 4),     # fbank512_wave_kernel<double, 8>
}


def grid_for_xcd(units, cus, per_cu):
    """host_common.hpp: grid_for, rounded up to a multiple of the eight XCDs"""
    g = min(units, cus * per_cu) or 1
    return (g + 7) // 8 * 8


def partition(family, n_units, cus):
    """-> (grid, waves of the grid, units per wave's run, waves with a unit) of a plain launch of n_units units"""
    waves, per_cu, _ = FAMILIES[family]
    grid = grid_for_xcd((n_units + waves - 1) // waves, cus, per_cu)
    total = grid * waves
    run = (n_units + total - 1) // total
    return grid, total, run, (n_units + run - 1) // run


def full_grid_waves(family, cus):
    waves, per_cu, _ = FAMILIES[family]
    return cus * per_cu * waves


def edge_batch(family, edge, cus, min_units=0):
    """(n_clips, units per clip) of a uniform batch at one edge of the partition (k x grid x waves + 1: at least min_units)"""
    G = full_grid_waves(family, cus)
    if edge == "fewer":                 # fewer units than waves: the grid is smaller than the CU count
        return 5, 23
    if edge == "exact":                 # exactly grid x waves units
        u = next(u for u in (64, 48, 32, 16, 8, 4, 2, 1) if G % u == 0)
        return G // u, u
    if edge == "plus1":                 # k x grid x waves + 1: the last busy wave has a partial run, the ones after it are idle
        for k in range(max(1, -(-min_units // G)), 9):
            t = k * G + 1
            for u in range(400, 6, -1):
                if t % u == 0:
                    return t // u, u
        raise AssertionError(f"no factor of k x {G} + 1")
    if edge == "inside":                # runs of 3 units, clips of 37: run boundaries fall inside clips
        return (2 * G + G // 3) // 37, 37
    raise ValueError(edge)


def edge_facts(family, n_units, cus):
    grid, total, run, busy = partition(family, n_units, cus)
    assert grid <= cus * FAMILIES[family][1] and grid % 8 == 0
    return dict(units=n_units, grid=grid, waves=total, run=run, busy=busy, ratio=round(n_units / full_grid_waves(family, cus), 4))


# ---- the fenced runner ------------------------------------------------------------------------------------------------------------

class Fence:
    """An output of n floats inside an allocation of n + 2 GUARD floats, all of it the sentinel before the call."""

    def __init__(self, gpu, n):
        self.n = int(n)
        self.buf = gpu.DeviceBuffer((self.n + 2 * GUARD) * 4)
        self.buf.upload(np.full(self.n + 2 * GUARD, SENTINEL, np.uint32))
        self.ptr = self.buf.ptr + GUARD * 4

    def bits(self):
        """the output's bits, after asserting (a): both guard bands are bit-for-bit intact"""
        raw = self.buf.download(self.n + 2 * GUARD, np.uint32)
        self.buf.free()
        lo, hi = raw[:GUARD], raw[GUARD + self.n:]
        assert np.all(lo == SENTINEL), f"write below the output: {int(np.sum(lo != SENTINEL))} words of the lower guard band changed"
        assert np.all(hi == SENTINEL), f"write past the output: {int(np.sum(hi != SENTINEL))} words of the upper guard band changed " \
                                       f"(first at +{int(np.argmax(hi != SENTINEL))})"
        return raw[GUARD:GUARD + self.n]


def _no_sentinel(bits, what):
    """(b): every word where a frame belongs was written"""
    left = bits == SENTINEL
    assert not left.any(), f"{what}: {int(left.sum())} words never written (first at word {int(np.argmax(left))})"


def _compare(got, want, tol, what):
    """every frame of every clip; got / want: lists of [frames, mels] (or [mels, cols]) per clip -> the worst difference"""
    worst, where, over = 0.0, None, None
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, (what, c, g.shape, w.shape)
        if w.size == 0:
            continue
        t = tol[c] if np.ndim(tol) else tol
        d = np.abs(g.astype(np.float64) - w.astype(np.float64))
        d[np.isnan(d)] = np.inf
        i = int(np.argmax(d))
        here = (c,) + tuple(int(v) for v in np.unravel_index(i, d.shape))
        if d.flat[i] > worst:
            worst, where = float(d.flat[i]), here
        if d.flat[i] > t and over is None:
            over = (float(d.flat[i]), t, here)
    assert over is None, f"{what}: |diff| {over[0]:.3e} > {over[1]:.1e} at (clip, frame, mel) = {over[2]}; worst {worst:.3e} at {where}"
    return worst


def _noise(n_clips, n, base=0):
    from oracle import oracle as O
    return np.stack([O.synth_pcm(base + c, n) for c in range(n_clips)]) if n_clips else np.zeros((0, n), np.float32)


def _upload(gpu, a):
    b = gpu.DeviceBuffer(max(a.nbytes, 16))
    b.upload(np.ascontiguousarray(a))
    return b


def run_uniform(gpu, m, clips, nm):
    n_clips, n = clips.shape
    nf = m.num_frames(n)
    pcm, out = _upload(gpu, clips), Fence(gpu, n_clips * nf * nm)
    m.compute_uniform_device(pcm.ptr, n, n, n_clips, out.ptr)
    m.synchronize()
    bits = out.bits()
    pcm.free()
    _no_sentinel(bits, "uniform")
    return list(bits.view(np.float32).reshape(n_clips, nf, nm))


def run_interleaved(gpu, m, clips, nm, major_column_order, min_width):
    """the padded ([W][mel], major_column_order) and mel-major ([mel][W]) layouts -> the frames of each clip as [frames, mels]"""
    n_clips, n = clips.shape
    nf, W = m.num_frames(n), m.interleaved_width(n, min_width)
    assert W > nf
    pcm, out = _upload(gpu, clips), Fence(gpu, n_clips * W * nm)
    m.compute_uniform_device_interleaved(pcm.ptr, n, n, n_clips, out.ptr, major_column_order, min_width)
    m.synchronize()
    bits = out.bits()
    pcm.free()
    _no_sentinel(bits, "layout")
    img = bits.view(np.float32).reshape((n_clips, W, nm) if major_column_order else (n_clips, nm, W))
    frames = img[:, :nf, :] if major_column_order else img[:, :, :nf].transpose(0, 2, 1)
    pad = img[:, nf:, :] if major_column_order else img[:, :, nf:]
    assert np.all(pad == 0.0), f"layout padding: {int(np.sum(pad != 0.0))} values are not 0.0"          # (c)
    return list(frames)


def ragged_lengths(n_fft, hop, n_clips, n_max, seed):
    """clip lengths of a ragged batch: runs of empty clips, n_fft - 1, n_fft, n_fft + hop, and lengths up to n_max"""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(n_fft, n_max + 1, n_clips)]
    special = [0, 0, 0, 0, n_fft - 1, n_fft, n_fft + hop, 0, 0, 0, n_fft + hop - 1, n_max, n_fft]
    for i, v in enumerate(special):
        lens[(i * 7 + 3) % n_clips] = v
    lens[-3:] = [0, 0, 0]
    lens[:3] = [0, 0, 0]
    return lens


def ragged_table(lens, frames, nm, gaps):
    """sample offsets (packed) and output offsets in floats; gaps: a multiple-of-four gap before some outputs"""
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    oo, cur, gap_spans = [], 0, []
    for c, f in enumerate(frames):
        g = (4 * (c % 3) + (nm if c % 5 == 0 else 0)) if gaps else 0
        if g:
            gap_spans.append((cur, cur + g))
        cur += g
        oo.append(cur)
        cur += f * nm
    return offs, np.array(oo, np.uint64), cur, gap_spans


def run_ragged(gpu, obj, flat, lens, frames, nm, gaps=True):
    offs, oo, total, gap_spans = ragged_table(lens, frames, nm, gaps)
    pcm, out = _upload(gpu, flat), Fence(gpu, total)
    obj.compute_ragged_device(pcm.ptr, offs, np.array(lens, np.uint64), out.ptr, oo)
    obj.synchronize()
    bits = out.bits()
    pcm.free()
    for a, b in gap_spans:                                                                                  # (d)
        assert np.all(bits[a:b] == SENTINEL), f"ragged: a gap between outputs at [{a}, {b}) was written"
    got = []
    for o, f in zip(oo, frames):
        _no_sentinel(bits[int(o):int(o) + f * nm], "ragged")
        got.append(bits[int(o):int(o) + f * nm].view(np.float32).reshape(f, nm))
    return got


def run_ragged_desc(gpu, obj, flat, lens, frames, nm, slack):
    """the clip table in device memory, packed outputs, max_total_frames = the truth + slack: the frames past the truth stay untouched"""
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    total = int(sum(frames))
    pcm, d_off, d_len = _upload(gpu, flat), _upload(gpu, offs), _upload(gpu, np.array(lens, np.uint64))
    out = Fence(gpu, (total + slack) * nm)
    obj.compute_ragged_device_desc(pcm.ptr, d_off.ptr, d_len.ptr, len(lens), out.ptr, 0, total + slack)
    obj.synchronize()
    bits = out.bits()
    for b in (pcm, d_off, d_len):
        b.free()
    _no_sentinel(bits[:total * nm], "ragged_desc")
    assert np.all(bits[total * nm:] == SENTINEL), "ragged_desc: a write past the last frame (inside max_total_frames)"
    got, cur = [], 0
    for f in frames:
        got.append(bits[cur:cur + f * nm].view(np.float32).reshape(f, nm))
        cur += f * nm
    return got


# ---- oracles ----------------------------------------------------------------------------------------------------------------------

def mel_oracle(oracle, clips, geo):
    fft, hop, sr, nm = geo
    return list(oracle.compute_mel_batch(clips, fft, hop, nm, sr, THREADS))


def _pmap(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(fn, items))


# ---- the dispatch matrix ----------------------------------------------------------------------------------------------------------

G80, G64, G40, G128, G60, G84, G100 = ((400, 160, SR, n) for n in (80, 64, 40, 128, 60, 84, 100))
G512 = (512, 160, SR, 80)

N = {   # the literals of melspec_plain_kernel_name, by the geometry and mode that reach them
    "six80": "melspec::whisper400_six_runs_kernel<9, LensSix80>",
    "six64": "melspec::whisper400_six_wide_runs_kernel<9, LensSix64> (twelve waves)",
    "six40": "melspec::whisper400_six_wide_runs_kernel<9, LensSix40> (twelve waves)",
    "sixrt": "melspec::whisper400_six_runs_kernel<9, LensRuntime>",
    "six128": "melspec::whisper400_six_wide_runs_kernel<15, LensSix128> (six frames per wave, twelve waves)",
    "wave8": "melspec::whisper400_wave_runs_kernel<8, .>",
    "wave12": "melspec::whisper400_wave_runs_kernel<12, .>",
}
GUARDED = {
    "six80": "melspec::whisper400_six_runs_kernel<9, LensSix80> (precision guard on)",
    "six64": "melspec::whisper400_six_wide_runs_kernel<9, LensSix64> (twelve waves; precision guard on)",
    "six40": "melspec::whisper400_six_wide_runs_kernel<9, LensSix40> (twelve waves; precision guard on)",
    "sixrt": "melspec::whisper400_six_runs_kernel<9, LensRuntime> (precision guard on)",
    "six128": "melspec::whisper400_six_wide_runs_kernel<15, LensSix128> (six frames per wave, twelve waves; precision guard on)",
    "wave8": "melspec::whisper400_wave_runs_kernel<8, .> (precision guard on)",
    "wave12": "melspec::whisper400_wave_runs_kernel<12, .> (precision guard on)",
}
F64N = {
    "six9": "melspec::whisper400_six64_kernel<9, .> (f64 FFT, six frames per wave, three waves per SIMD)",
    "six15": "melspec::whisper400_six64_kernel<15, LensSix128> (f64 FFT, six frames per wave, three waves per SIMD, fifteen mel slots)",
    "p8": "melspec::whisper400_precise_kernel<8, ., RUNS> (f64 FFT)",
    "p12": "melspec::whisper400_precise_kernel<12, ., RUNS> (f64 FFT)",
}
W512 = {
    "f32": "melspec::fbank512_wave_kernel<float, 12, 1, kFlavorWhisper, RUNS> (n_fft = 512, f32, three waves per SIMD)",
    "auto": "melspec::w512_auto_kernel<float, 12> (n_fft = 512, f32, precision guard + vote) + the gated melspec::w512_auto_kernel<double, 8>",
    "f64": "melspec::fbank512_wave_kernel<double, 8, 1, kFlavorWhisper, RUNS> (n_fft = 512, f64)",
}
POW2 = {
    6: "melspec::pow2_frame_kernel<6, kFlavorWhisper> (n_fft = 128, f64, frames owned by lane groups of a wave)",
    7: "melspec::pow2_frame_kernel<7, kFlavorWhisper> (n_fft = 256, f64, frames owned by lane groups of a wave)",
    8: "melspec::pow2_frame_kernel<8, kFlavorWhisper> (n_fft = 512, f64, frames owned by lane groups of a wave)",
    9: "melspec::pow2_frame_kernel<9, kFlavorWhisper> (n_fft = 1024, f64, frames owned by lane groups of a wave)",
    10: "melspec::pow2_frame_kernel<10, kFlavorWhisper> (n_fft = 2048 as two 512-point halves, f64, frames owned by lane groups of a wave)",
}
GENERIC = "melspec::generic_frame_kernel<256> (f64, one frame per workgroup)"


@dataclass
class Row:
    id: str
    geo: tuple                 # (n_fft, hop, sample rate, n_mels)
    prec: str | None           # None: the context's default mode (AUTO; F64 in the f64-initial pass); else set explicitly
    entry: str                 # uniform | ragged | ragged_desc | padded | melmajor
    batch: str                 # an edge of the partition (uniform), or "ragged" / "layout" / "small"
    name: str                  # what melspec_plain_kernel_name reports
    name64: str | None = None  # ... in the f64-initial pass (default-mode rows)
    family: str | None = None  # the partition of the plain launch (FAMILIES)
    extra: dict = field(default_factory=dict)


EDGES = ("fewer", "exact", "plus1", "inside")
ROWS = []
for key, geo, fam, f64 in (("six80", G80, "six16", "six9"), ("six64", G64, "six12", "six9"), ("six40", G40, "six12", "six9"),
                           ("six128", G128, "six12", "six15"), ("sixrt", G60, "six16", "six9"), ("wave8", G84, "wave", "p8"),
                           ("wave12", G100, "wave", "p12")):
    for e in EDGES:             # AUTO on every edge; the f64-initial pass runs the same batches on the f64 kernels
        ROWS.append(Row(f"{key}-auto-{e}", geo, None, "uniform", e, GUARDED[key], F64N[f64], fam))
    ROWS.append(Row(f"{key}-f32-plus1", geo, "f32", "uniform", "plus1", N[key], family=fam))
    ROWS.append(Row(f"{key}-auto-ragged", geo, None, "ragged", "ragged", GUARDED[key], F64N[f64]))
for key, geo, fam in (("six9", G80, "six64"), ("six15", G128, "six64"), ("p8", G84, "precise"), ("p12", G100, "precise")):
    for e in EDGES:
        ROWS.append(Row(f"{key}-f64-{e}", geo, "f64", "uniform", e, F64N[key], family=fam))
ROWS += [
    Row("six80-auto-desc", G80, None, "ragged_desc", "ragged", GUARDED["six80"], F64N["six9"]),
    Row("wave12-f32-desc", G100, "f32", "ragged_desc", "ragged", N["wave12"]),
    Row("six9-f64-ragged", G80, "f64", "ragged", "ragged", F64N["six9"]),
    Row("p12-f64-ragged", G100, "f64", "ragged", "ragged", F64N["p12"]),
    # the round-robin layout kernels behind each f32 kernel, and the f64 layout kernels
    Row("six80-auto-melmajor", G80, None, "melmajor", "layout", GUARDED["six80"], F64N["six9"]),
    Row("six80-f32-padded", G80, "f32", "padded", "layout", N["six80"]),
    Row("six64-auto-padded", G64, None, "padded", "layout", GUARDED["six64"], F64N["six9"]),
    Row("six40-f32-melmajor", G40, "f32", "melmajor", "layout", N["six40"]),
    Row("six128-auto-melmajor", G128, None, "melmajor", "layout", GUARDED["six128"], F64N["six15"]),
    Row("six128-f32-padded", G128, "f32", "padded", "layout", N["six128"]),
    Row("sixrt-auto-padded", G60, None, "padded", "layout", GUARDED["sixrt"], F64N["six9"]),
    Row("wave8-auto-melmajor", G84, None, "melmajor", "layout", GUARDED["wave8"], F64N["p8"]),
    Row("wave12-f32-padded", G100, "f32", "padded", "layout", N["wave12"]),
    Row("six9-f64-melmajor", G80, "f64", "melmajor", "layout", F64N["six9"]),
    Row("six15-f64-padded", G128, "f64", "padded", "layout", F64N["six15"]),
    Row("p8-f64-padded", G84, "f64", "padded", "layout", F64N["p8"]),
    Row("p12-f64-melmajor", G100, "f64", "melmajor", "layout", F64N["p12"]),
    # n_fft = 512: the vote needs more than 24 576 frames (k = 2 below); the f32 and f64 kernels
    Row("w512-auto-plus1", G512, None, "uniform", "plus1", W512["auto"], W512["f64"], "f512_32"),
    Row("w512-f32-plus1", G512, "f32", "uniform", "plus1", W512["f32"], family="f512_32"),
    Row("w512-f64-exact", G512, "f64", "uniform", "exact", W512["f64"], family="f512_64"),
    Row("w512-f64-plus1", G512, "f64", "uniform", "plus1", W512["f64"], family="f512_64"),
    Row("w512-auto-ragged", G512, None, "ragged", "ragged", W512["auto"], W512["f64"]),
    Row("w512-f32-melmajor", G512, "f32", "melmajor", "layout", W512["f32"]),
    # every geometry off the fused kernels
    Row("pow2-128", (128, 32, 8000.0, 20), None, "uniform", "small", POW2[6], POW2[6]),
    Row("pow2-256", (256, 64, 8000.0, 40), None, "ragged", "ragged", POW2[7], POW2[7]),
    Row("pow2-512", (512, 160, SR, 200), None, "uniform", "small", POW2[8], POW2[8]),
    Row("pow2-1024", (1024, 256, SR, 80), None, "padded", "layout", POW2[9], POW2[9]),
    Row("pow2-2048", (2048, 512, 44100.0, 128), None, "uniform", "small", POW2[10], POW2[10]),
    Row("generic-300", (300, 100, SR, 40), None, "uniform", "small", GENERIC, GENERIC),
    Row("generic-300-ragged", (300, 100, SR, 40), None, "ragged_desc", "ragged", GENERIC, GENERIC),
]


def _tol(row):
    if row.prec == "f32":
        return F32_TOL
    f64 = row.prec == "f64" or not _auto_pass() or row.name in (GENERIC, W512["f64"], *POW2.values())
    return F64_TOL if f64 else TOL


def _uniform_clips(row, cus):
    fft, hop, sr, nm = row.geo
    if row.batch == "small":
        return _noise(7, fft + 37 * hop + 11, 300)
    if row.batch == "layout":
        return _noise(37, fft + 200 * hop + 3, 400)          # 201 frames: odd, so min_width adds padding after the zero column
    fpu = FAMILIES[row.family][2]
    # n_fft = 512: AUTO votes on batches of more than 24 576 frames (smaller ones run on the f64 kernel)
    n_clips, u = edge_batch(row.family, row.batch, cus, 24576 // fpu + 1 if row.geo == G512 and row.prec != "f64" else 0)
    frames = u * fpu - (fpu // 2 if u > 1 else 0)          # the clip's last unit partial where it can be
    assert (frames + fpu - 1) // fpu == u
    return _noise(n_clips, fft + (frames - 1) * hop, 1000)


@pytest.mark.gpu
@pytest.mark.parametrize("row", ROWS, ids=lambda r: r.id)
def test_dispatch_matrix_whole_batch(gpu, oracle, row):
    if row.prec is not None and not _auto_pass():
        pytest.skip("a row with an explicit precision runs once, in the default-mode pass")
    cus = _cus()
    fft, hop, sr, nm = row.geo
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    if row.prec is not None:
        m.set_precision(row.prec)
    want_name = row.name if _auto_pass() else row.name64
    assert m.plain_kernel_name() == want_name, (m.plain_kernel_name(), want_name)
    facts = {}
    if row.entry in ("uniform", "padded", "melmajor"):
        clips = _uniform_clips(row, cus)
        want = mel_oracle(oracle, clips, row.geo)
        if row.entry == "uniform":
            got = run_uniform(gpu, m, clips, nm)
            if row.family and (_auto_pass() or row.prec is not None):
                u = (m.num_frames(clips.shape[1]) + FAMILIES[row.family][2] - 1) // FAMILIES[row.family][2]
                facts = edge_facts(row.family, u * clips.shape[0], cus)
                if row.batch == "fewer":
                    assert facts["grid"] < cus
                elif row.batch == "exact":
                    assert facts["units"] == facts["waves"] and facts["grid"] == cus * FAMILIES[row.family][1]
                elif row.batch == "plus1":
                    assert facts["units"] % facts["waves"] == 1 and facts["busy"] < facts["waves"]
                elif row.batch == "inside":
                    assert facts["run"] > 1 and u % facts["run"] != 0
        else:
            got = run_interleaved(gpu, m, clips, nm, row.entry == "padded", m.num_frames(clips.shape[1]) + 41)
    else:
        n_max = fft + 150 * hop
        lens = ragged_lengths(fft, hop, 160, n_max, 7)
        base = _noise(len(lens), n_max, 2000)
        full = mel_oracle(oracle, base, row.geo)
        frames = [m.num_frames(n) for n in lens]
        want = [f[:k] for f, k in zip(full, frames)]
        flat = np.concatenate([b[:n] for b, n in zip(base, lens)])
        if row.entry == "ragged":
            got = run_ragged(gpu, m, flat, lens, frames, nm)
        else:
            got = run_ragged_desc(gpu, m, flat, lens, frames, nm, slack=5000)
    worst = _compare(got, want, _tol(row), row.id)
    print(f"\nWHOLE-BATCH {row.id}: {m.plain_kernel_name()} frames={sum(w.shape[0] for w in want)} worst={worst:.3e} "
          f"guard={m.guard_last_count() if m.precision == 'auto' else '-'} {facts}")
    m.close()


# ---- Kaldi fbank and the NeMo frontend -------------------------------------------------------------------------------------------

FBANK_ROWS = ["clip-kernel", "fused-cmn", "split", "ragged", "generic-8k"]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", FBANK_ROWS)
def test_fbank_whole_batch(gpu, oracle, kind):
    cus = _cus()
    sr = 8000.0 if kind == "generic-8k" else SR
    fb = gpu.Fbank(gpu.FbankConfig(sample_rate=sr))
    oc = oracle.fbank_default_config()
    oc.sample_rate = sr
    assert fb.uses_fast_path == (kind != "generic-8k")
    nm = fb.num_mel_bins
    if kind == "ragged":
        fl, fs = 400, 160
        lens = ragged_lengths(fl, fs, 140, fl + 120 * fs, 9)
        base = _noise(len(lens), max(lens), 3000)
        clips = [b[:n] for b, n in zip(base, lens)]
        frames = [fb.num_frames(n) for n in lens]
        got = run_ragged(gpu, fb, np.concatenate(clips), lens, frames, nm)
        want = _pmap(lambda x: oracle.fbank_compute(x, oc), clips)
    else:
        # the workgroup-per-clip kernel wants at least one clip per CU (2 x cus here); small batches take the fused kernel + cmn_kernel
        n_clips = {"clip-kernel": 2 * cus, "fused-cmn": 5, "split": 2 * cus + 3, "generic-8k": 9}[kind]
        n = {"clip-kernel": 16000, "fused-cmn": 64000 + 77, "split": 16000, "generic-8k": 24000}[kind]
        clips = _noise(n_clips, n, 4000)
        want = list(oracle.fbank_batch(clips, oc, THREADS))
        nf = fb.num_frames(n)
        pcm = _upload(gpu, clips)
        if kind == "split":
            rows, means = Fence(gpu, n_clips * nf * nm), Fence(gpu, n_clips * nm)
            fb.compute_uniform_device_split(pcm.ptr, n, n, n_clips, rows.ptr, means.ptr)
            fb.synchronize()
            rb, mb = rows.bits(), means.bits()
            _no_sentinel(rb, "split rows"); _no_sentinel(mb, "split means")
            r3 = rb.view(np.float32).reshape(n_clips, nf, nm)
            m2 = mb.view(np.float32).reshape(n_clips, 1, nm)
            got = list((r3 - m2).astype(np.float32))
        else:
            out = Fence(gpu, n_clips * nf * nm)
            fb.compute_uniform_device(pcm.ptr, n, n, n_clips, out.ptr)
            fb.synchronize()
            bits = out.bits()
            _no_sentinel(bits, kind)
            got = list(bits.view(np.float32).reshape(n_clips, nf, nm))
        pcm.free()
    worst = _compare(got, want, TOL, f"fbank {kind}")
    print(f"\nWHOLE-BATCH fbank-{kind}: frames={sum(w.shape[0] for w in want)} worst={worst:.3e}")
    fb.close()


NEMO_ROWS = [("f64", False, 0), ("f64", True, 0), ("f64", False, 16), ("f32", False, 0), ("f32", True, 16), ("f64", True, 16)]


@pytest.mark.gpu
@pytest.mark.parametrize("prec,norm,pad_to", NEMO_ROWS, ids=lambda v: str(v))
def test_nemo_whole_batch(gpu, oracle, prec, norm, pad_to):
    if prec == "f32" and not _auto_pass():
        pytest.skip("a row with an explicit precision runs once, in the default-mode pass")
    kw = dict(n_mels=128 if pad_to else 80, preemphasis=0.97, log_zero_guard=2.0 ** -24, normalize_per_feature=norm, pad_to=pad_to)
    fe = gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))
    if prec == "f32":
        fe.set_precision("f32")
    cfg = oracle.blm_default_config(**kw)
    n_clips, n = _cus() + 5, 16000 + 37
    clips = _noise(n_clips, n, 5000)
    cols, nm = fe.padded_frames(n), kw["n_mels"]
    valid = fe.num_frames(n)
    assert (cols > valid) == (pad_to > 0)
    pcm, out = _upload(gpu, clips), Fence(gpu, n_clips * nm * cols)
    fe.compute_uniform_device(pcm.ptr, n, n, n_clips, out.ptr)
    fe.synchronize()
    bits = out.bits()
    pcm.free()
    _no_sentinel(bits, "nemo")
    got = bits.view(np.float32).reshape(n_clips, nm, cols)
    want = _pmap(lambda x: oracle.blm_compute(x, cfg, True)[0], list(clips))
    if pad_to:                                                                                              # (c)
        pads = np.stack([w[:, valid:] for w in want])
        assert np.array_equal(got[:, :, valid:], pads), "NeMo pad_to columns differ from the oracle's"
    tol = TOL
    if prec == "f32":
        # tests/test_f32_512.py's gate of this mode: as far from the f64 evaluation as the reference's literal f32 arithmetic is (4 x its
        # distance, per clip), and on noise-like input within 1.5e-4 whatever that distance
        lit = _pmap(lambda x: oracle.blm_compute(x, cfg, False)[0], list(clips))
        tol = [max(1.5 * TOL, 4.0 * float(np.abs(a.astype(np.float64) - w).max())) for a, w in zip(lit, want)]
    worst = _compare(list(got), want, tol, f"nemo {prec} norm={norm} pad_to={pad_to}")
    print(f"\nWHOLE-BATCH nemo-{prec}-norm{int(norm)}-pad{pad_to}: frames={n_clips * valid} worst={worst:.3e}")
    fe.close()


# ---- AUTO's contract, per frame ---------------------------------------------------------------------------------------------------

def light_batch(family, fft, hop, cus, seed):
    """hash noise in one-unit clips, 2.5 x grid x waves units (runs of 2-3 units); about 3 % of the clips a line 70 .. 90 dB over its
    floor: the last clip and clips that hold the middle of a wave's run, so that the vote's sample (the first unit of every wave) does
    not see them -> (clips, indices of the hard clips)"""
    fpu = FAMILIES[family][2]
    G = full_grid_waves(family, cus)
    n_units = 2 * G + G // 2 + 1
    n = fft + (fpu - 1) * hop
    clips = _noise(n_units, n, 7000 + seed)
    _, _, run, busy = partition(family, n_units, cus)
    assert run >= 2
    hard = sorted(set([w * run + run // 2 for w in range(0, busy, 11) if w * run + run // 2 < n_units] + [n_units - 1]))
    rng = np.random.default_rng(seed)
    for i, c in enumerate(hard):
        clips[c] = _tone_over_floor(n, -70.0 - 20.0 * rng.random(), 300.0 + 7000.0 * rng.random(), 100 * seed + i)
    assert 0.02 <= len(hard) / n_units <= 0.05, len(hard) / n_units
    return clips, hard


AUTO_ROWS = [("six80", G80, "six16", "uniform"), ("six64", G64, "six12", "uniform"), ("six40", G40, "six12", "uniform"),
             ("six128", G128, "six12", "uniform"), ("sixrt", G60, "six16", "uniform"), ("six80", G80, "six16", "melmajor")]


@pytest.mark.gpu
@pytest.mark.parametrize("key,geo,family,entry", AUTO_ROWS, ids=lambda v: v if isinstance(v, str) else None)
def test_auto_light_batch_per_frame(gpu, oracle, key, geo, family, entry):
    """Every AUTO frame is the f32 kernel's frame bit for bit, or within 2e-6 of the oracle (recomputed in f64); every frame the bare
    f32 kernel misses by more than 1e-4 is of the second kind; every frame within 1e-4."""
    if not _auto_pass():
        pytest.skip("AUTO's contract: the default-mode pass")
    cus = _cus()
    fft, hop, sr, nm = geo
    clips, hard = light_batch(family, fft, hop, cus, {"six80": 1, "six64": 2, "six40": 3, "six128": 4, "sixrt": 5}[key])
    m = gpu.HipMelSpectrogram(fft, hop, sr, nm)
    assert m.plain_kernel_name() == GUARDED[key]

    def run():
        if entry == "uniform":
            return np.stack(run_uniform(gpu, m, clips, nm))
        return np.stack(run_interleaved(gpu, m, clips, nm, False, m.num_frames(clips.shape[1]) + 2))

    m.guard_last_count()
    auto = run()
    heavy, frac = m.auto_state()
    noted = m.guard_last_count()
    assert not heavy and noted > 0, (heavy, frac, noted)
    m.set_precision("f32")
    bare = run()
    m.close()
    want = np.stack(mel_oracle(oracle, clips, geo))
    d_auto = np.abs(auto.astype(np.float64) - want).max(axis=2)
    d_bare = np.abs(bare.astype(np.float64) - want).max(axis=2)
    same = np.all(auto.view(np.uint32) == bare.view(np.uint32), axis=2)
    recomputed = d_auto <= F64_TOL
    _compare(list(auto), list(want), TOL, f"AUTO {key} {entry}")
    bad = ~(same | recomputed)
    assert not bad.any(), f"{int(bad.sum())} AUTO frames neither the f32 frame nor f64-accurate, first (clip, frame) " \
                          f"{tuple(int(v) for v in np.argwhere(bad)[0])}, |diff| {float(d_auto[bad].max()):.3e}"
    missed = d_bare > TOL
    assert np.all(recomputed[missed]), f"{int((missed & ~recomputed).sum())} frames the f32 kernel misses were not recomputed"
    print(f"\nWHOLE-BATCH auto-light {key} {entry}: frames={want.shape[0] * want.shape[1]} hard={len(hard)} noted={noted} "
          f"recomputed(not bit-equal)={int((~same).sum())} f32-missed={int(missed.sum())} worst={float(d_auto.max()):.3e}")


@pytest.mark.gpu
def test_auto_heavy_batch_per_frame(gpu, oracle, jfk):
    """speech: the vote sends the batch to the f64 kernel; every frame within 2e-6"""
    if not _auto_pass():
        pytest.skip("AUTO's contract: the default-mode pass")
    n_clips, n = 300, 400 + 99 * 160
    clips = np.stack([np.resize(np.roll(jfk, -2311 * c), n) for c in range(n_clips)])
    m = gpu.HipMelSpectrogram(*G80)
    got = run_uniform(gpu, m, clips, 80)
    assert m.auto_state()[0]
    worst = _compare(got, mel_oracle(oracle, clips, G80), F64_TOL, "AUTO heavy")
    print(f"\nWHOLE-BATCH auto-heavy: frames={n_clips * 100} worst={worst:.3e}")
    m.close()


@pytest.mark.gpu
def test_auto_512_light_batch_per_frame(gpu, oracle):
    """w512_auto_kernel: every frame within 1e-4; every frame the f32 kernel misses by more than 1e-4 within 3e-6 (recomputed)"""
    if not _auto_pass():
        pytest.skip("AUTO's contract: the default-mode pass")
    cus = _cus()
    clips, hard = light_batch("f512_32", 512, 160, cus, 6)
    assert clips.shape[0] * 4 > 24576
    m = gpu.HipMelSpectrogram(*G512)
    assert m.plain_kernel_name() == W512["auto"]
    m.guard_last_count()
    auto = np.stack(run_uniform(gpu, m, clips, 80))
    heavy, frac = m.auto_state()
    noted = m.guard_last_count()
    assert not heavy and noted > 0, (heavy, frac, noted)
    m.set_precision("f32")
    bare = np.stack(run_uniform(gpu, m, clips, 80))
    m.close()
    want = np.stack(mel_oracle(oracle, clips, G512))
    _compare(list(auto), list(want), TOL, "AUTO 512")
    d_auto = np.abs(auto.astype(np.float64) - want).max(axis=2)
    missed = np.abs(bare.astype(np.float64) - want).max(axis=2) > TOL
    assert np.all(d_auto[missed] <= 3e-6), f"{int((d_auto[missed] > 3e-6).sum())} frames the f32 kernel misses are not f64-accurate " \
                                           f"(worst {float(d_auto[missed].max()):.3e})"
    print(f"\nWHOLE-BATCH auto-512-light: frames={want.shape[0] * want.shape[1]} hard={len(hard)} noted={noted} "
          f"f32-missed={int(missed.sum())} worst={float(d_auto.max()):.3e}")


@pytest.mark.gpu
def test_auto_state_does_not_leak_into_the_next_batch(gpu, oracle):
    """a large light batch with hard clips, then a small noise batch in another layout on the same context: the same bits as on a
    fresh context (no notes, no vote words of the previous launch)"""
    if not _auto_pass():
        pytest.skip("AUTO's contract: the default-mode pass")
    cus = _cus()
    clips, _ = light_batch("six16", 400, 160, cus, 8)
    small = _noise(3, 400 + 60 * 160, 9000)
    m = gpu.HipMelSpectrogram(*G80)
    run_uniform(gpu, m, clips, 80)
    assert m.guard_last_count() > 0
    after = np.stack(run_interleaved(gpu, m, small, 80, False, 80))
    m.close()
    fresh_ctx = gpu.HipMelSpectrogram(*G80)
    fresh = np.stack(run_interleaved(gpu, fresh_ctx, small, 80, False, 80))
    fresh_ctx.close()
    assert np.array_equal(after.view(np.uint32), fresh.view(np.uint32))
    _compare(list(after), mel_oracle(oracle, small, G80), TOL, "small batch after a large one")


# ---- the matrix against the source (CPU) ------------------------------------------------------------------------------------------

def plain_kernel_name_literals():
    """the strings melspec_plain_kernel_name hands out: the names of the n_fft = 400 routes (ctx_route.hpp) and of the two families off them"""
    csrc = os.path.join(ROOT, "mel_spec_amd", "csrc")
    found = set()
    for file, heads in (("ctx_route.hpp", ("inline const char *route_name(F32Kernel k, bool guarded) {", "inline const char *route_name(F64Kernel k) {")),
                        ("fused512_route.hpp", ("inline const char *whisper512_kernel_name(const Fused512Shape &s) {",)),
                        ("pow2.hip", ("const char *generic_kernel_name(const GenericTables &gt) {",))):
        src = open(os.path.join(csrc, file)).read()
        for head in heads:
            start = src.index(head)
            body = src[start:src.index("\n}\n", start)]
            found |= {s for s in re.findall(r'"((?:[^"\\]|\\.)*)"', body) if s}
    return found


def test_whole_batch_matrix_names_every_plain_kernel():
    """every string melspec_plain_kernel_name can return has a row in the whole-batch matrix, and no row names one it cannot return"""
    literals = plain_kernel_name_literals()
    assert len(literals) >= 27, sorted(literals)
    named = {r.name for r in ROWS} | {r.name64 for r in ROWS if r.name64}
    assert not named - literals, f"rows name kernels melspec_plain_kernel_name does not return: {sorted(named - literals)}"
    assert not literals - named, f"kernels without a whole-batch row: {sorted(literals - named)}"
    for r in ROWS:
        assert r.entry in ("uniform", "ragged", "ragged_desc", "padded", "melmajor"), r.id
        assert r.entry != "uniform" or r.batch == "small" or r.family in FAMILIES, r.id


def test_whole_batch_partition_edges():
    """the sizes the matrix picks land on the edges they claim, on any CU count"""
    for cus in (256, 304, 80):
        for fam in FAMILIES:
            G = full_grid_waves(fam, cus)
            for e in EDGES:
                n_clips, u = edge_batch(fam, e, cus)
                f = edge_facts(fam, n_clips * u, cus)
                if e == "fewer":
                    assert f["grid"] < cus and f["units"] < f["waves"]
                elif e == "exact":
                    assert f["units"] == f["waves"] == G
                elif e == "plus1":
                    assert f["units"] % G == 1 and f["busy"] < f["waves"]
                else:
                    assert f["run"] == 3 and u % 3 != 0
