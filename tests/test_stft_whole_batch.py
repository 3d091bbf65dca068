"""Whole batches through the split API -- the STFT export, the mel stage on spectra, streaming spectra -- every frame of every clip
against the oracle, in fenced buffers.

The reference's split API is Spectrogram::compute_all_cpu / Spectrogram::add (src/stft.rs:48-115), then MelSpectrogram::add(&fft)
(src/mel.rs:13-32); here melspec_stft_uniform_device / _ragged_device / _host, melspec_mel_from_stft_device and
melspec_stream_push_host_stft.  tests/test_whole_batch.py gives the fused kernels this treatment; this file gives it to

  whisper400_stft_kernel   (whisper400_kernels.hpp)  a ClipRun per wave: batches on the four edges of the run-per-wave partition;
  generic_stft_kernel      (generic_kernels.hpp)     radix-2, mixed-radix and direct-DFT transforms, below / at / past the grid cap;
  mel_stage_jobs_kernel, mel_stage_kernel<T, 4>  (aux_kernels.hpp)  more frames than two trips of every wave of a full grid;
  a stream bank's pushes of spectra, several streams per push (a ragged STFT launch over the bank's state buffer).

A complex output is a run of 32-bit words (2 x bins per frame for complex64, 4 x bins for complex128), so Fence and the sentinel of
tests/test_whole_batch.py serve as they are.  Every test asserts: the guard bands are intact, no sentinel is left where a frame
belongs, the gaps between ragged outputs still hold the sentinel, and EVERY frame passes the gate:

  complex128   |got - want| <= 1e-10 x ||want frame||_2                                (test_stft_export_matches_compute_all_cpu's)
  complex64    the f64 result rounded once: per real and per imaginary component
               |got - want| <= 1e-10 x ||want frame||_2 + 2^-24 x |want component|     (the gate above + half an ulp)
  mel rows     2e-6 on f64 spectra, 1e-4 on f32 spectra                                (test_mel_stage_on_stft_frames')

want = oracle.compute_all_cpu (f64; pinned to numpy.fft at 1e-13 x the frame norm by the CPU test at the end), ||want frame||_2 the
norm of its n_fft bins, as in the existing test.  Two properties of the GPU's own output are exact: in the full layout bin n_fft - k
is bit for bit the conjugate of bin k (the kernels store re, -im of the same registers), and bins 0 .. n_fft/2 of the full call are bit
for bit the half call's (one kernel, `bins` a run-time value)."""
import ctypes as C

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py)

from test_whole_batch import (FAMILIES, SENTINEL, SR, THREADS, Fence, _cus, _no_sentinel, _noise, _pmap, _upload, edge_batch, edge_facts,
                              partition, ragged_lengths)

GATE64 = 1e-10               # x the frame's 2-norm
HALF_ULP32 = 2.0 ** -24      # x |component|
MEL_TOL = {True: 2e-6, False: 1e-4}     # by f64 spectra
WORDS = {True: 4, False: 2}             # 32-bit words per complex element, by f64
CDT = {True: np.complex128, False: np.complex64}
SENTINEL64 = np.uint64(int(SENTINEL) << 32 | int(SENTINEL))
EDGES = ("fewer", "exact", "plus1", "inside")
ERR_CAPACITY = -3            # include/melspec_hip.h
HOST_GUARD = 64              # words either side of a fenced host array (256 bytes: the array keeps its alignment)

W400 = (400, 160, 80)
GENERIC = {"radix2": (256, 64, 40), "mixed": (300, 100, 40), "direct": (441, 160, 64)}
GENERIC_BATCHES = ("below", "cap", "cap+1", "past")
STAGE = {"80": (400, 160, 80), "128": (400, 160, 128), "512bins": (1024, 256, 80)}
STAGE_FALLBACK = ((512, 160, 300), (1024, 256, 300))
STREAM_CASES = [(400, 160, True, True), (400, 160, False, False), (512, 160, False, True), (441, 160, True, False)]
PIN_GEOMETRIES = [(400, 160), (256, 64), (300, 100), (441, 160), (98, 40), (512, 160), (1024, 256)]


def _label(f64, full):
    return f"{'c128' if f64 else 'c64'}-{'full' if full else 'half'}"


# ---- the batch recipes (arithmetic on the CU count only: the CPU test at the end restates them) ------------------------------------

def whisper_batch(edge, cus):
    """-> (n_clips, units per clip, frames per clip) of a uniform batch of whisper400_stft_kernel at one edge of the partition of the
    `precise` family (8 waves, one workgroup per CU, 5 frames per unit); the clip's last unit partial where it can be"""
    n_clips, u = edge_batch("precise", edge, cus)
    fpu = FAMILIES["precise"][2]
    frames = u * fpu - (2 if u > 1 else 0)
    assert (frames + fpu - 1) // fpu == u
    return n_clips, u, frames


def check_edge(edge, facts, u, cus):
    if edge == "fewer":
        assert facts["grid"] < cus
    elif edge == "exact":
        assert facts["units"] == facts["waves"]
    elif edge == "plus1":
        assert facts["units"] % facts["waves"] == 1 and facts["busy"] < facts["waves"]
    else:
        assert facts["run"] > 1 and u % facts["run"] != 0


def generic_batch(kind, cus):
    """-> (n_clips, frames per clip) around launch_generic_stft's grid cap of 8 x CUs workgroups (pow2.hip), a frame per workgroup trip"""
    cap = 8 * cus
    if kind == "below":
        return 7, 37
    if kind == "cap":
        return 8, cus
    if kind == "cap+1":
        d = next((d for d in range(7, 1, -1) if (cap + 1) % d == 0), 1)
        return d, (cap + 1) // d
    if kind == "past":                       # about 2.3 trips, clips of 37 frames: the trip boundaries fall inside clips
        return int(2.3 * cap) // 37, 37
    raise ValueError(kind)


def check_generic_batch(kind, total, cus):
    cap = 8 * cus
    assert {"below": total < cap, "cap": total == cap, "cap+1": total == cap + 1, "past": 2 * cap < total < 3 * cap and cap % 37 != 0}[kind]


def stage_f1(cus):
    return 2 * cus * 32 + 13


def stage_f2(cus):
    return 2 * cus * 64 + 5


def stage_rule(oracle, n_fft, n_mels, sr=SR):
    """melspec_mel_from_stft_device's choice (mel_spec_amd/csrc/aux.hip): mel_stage_jobs_kernel iff n_jobs > 0 && n_mels <= 256 &&
    bin_limit <= 4088 && lds <= 64 KiB, on a grid of at most CUs x min(4, 160 KiB / lds) workgroups of eight waves; else
    mel_stage_kernel<T, 4> on at most CUs x 16 workgroups of four.  -> (takes the jobs kernel, its workgroups per CU, its LDS bytes).
    A RESTATEMENT: n_jobs follows build_mel_jobs (jobs of eight bins from an even one per band, sets of sixteen, two sets per 32 lanes),
    the LDS size mel_stage_lds (aux_kernels.hpp), the bank is the oracle's.  Nothing observes which kernel really ran -- the library has
    no hook for it.  If the rule in aux.hip changes, this function has to change with it; otherwise the tests below go on passing while
    their frame counts no longer reach the second trip of the kernel they name."""
    lim = n_fft // 2
    fb = oracle.mel_filterbank(sr, n_fft, n_mels)[:, :lim]
    nj = 0
    for m in range(min(n_mels, 256)):
        nz = np.flatnonzero(fb[m])
        if nz.size:
            nj += len(range(int(nz[0]) & ~1, int(nz[-1]) + 1, 8))
    sets = max(1, -(-nj // 16))
    n_jobs = (sets + 1) // 2 * 32 if nj else 0
    frames_at = (8 * n_jobs + (n_jobs + 1) // 2 + 31) & ~31
    acc_at = (lim + 8 + 1) & ~1
    lds = 8 * (frames_at + 8 * ((acc_at + n_mels + 31) & ~31))
    takes = n_jobs > 0 and n_mels <= 256 and lim <= 4088 and lds <= 64 * 1024
    return takes, max(1, min(4, 160 * 1024 // lds)), lds


# ---- references: computed once, shared, read-only ----------------------------------------------------------------------------------

_REF = {}


def _once(key, make):
    if key not in _REF:
        v = make()
        for a in (v if isinstance(v, list) else [v]):
            a.setflags(write=False)
        _REF[key] = v
    return _REF[key]


def stft_ref(oracle, key, clips, fft, hop):
    """compute_all_cpu of every clip of a batch -> list of [frames][n_fft] complex128"""
    return _once(("stft", key, fft, hop), lambda: _pmap(lambda x: oracle.compute_all_cpu(x, fft, hop), list(clips)))


def _segments(n_frames, k=512):
    return [(a, min(a + k, n_frames)) for a in range(0, n_frames, k)]


def stft_ref_long(oracle, key, x, fft, hop):
    """compute_all_cpu of one long clip, its frames dealt to the pool in segments"""
    nf = oracle.num_frames(len(x), fft, hop)
    return _once(("stft-long", key, fft, hop), lambda: np.concatenate(
        _pmap(lambda ab: oracle.compute_all_cpu(x[ab[0] * hop:(ab[1] - 1) * hop + fft], fft, hop), _segments(nf))))


def mel_ref_long(oracle, key, x, fft, hop, nm):
    """the oracle's fused pipeline on one long clip: each frame's row depends on that frame alone, so segments of frames are clips of a batch"""
    def make():
        nf = oracle.num_frames(len(x), fft, hop)
        segs = _segments(nf, 1024)
        whole = [s for s in segs if s[1] - s[0] == 1024]
        parts = []
        if whole:
            batch = np.stack([x[a * hop:(b - 1) * hop + fft] for a, b in whole])
            parts.append(oracle.compute_mel_batch(batch, fft, hop, nm, SR, THREADS).reshape(-1, nm))
        if len(whole) < len(segs):
            a, b = segs[-1]
            parts.append(oracle.compute_mel_spectrogram_cpu(x[a * hop:(b - 1) * hop + fft], fft, hop, nm, SR))
        return np.concatenate(parts)
    return _once(("mel-long", key, fft, hop, nm), make)


# ---- the gates ---------------------------------------------------------------------------------------------------------------------

def gate_ratio(got, want_full, f64):
    """got [frames][bins] of one clip, want_full [frames][n_fft] -> each element's distance as a fraction of its gate"""
    w = want_full[:, :got.shape[1]]
    base = GATE64 * np.linalg.norm(want_full, axis=1)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        if f64:
            r = np.abs(got - w) / base
        else:
            g = got.astype(np.complex128)
            r = np.maximum(np.abs(g.real - w.real) / (base + HALF_ULP32 * np.abs(w.real)),
                           np.abs(g.imag - w.imag) / (base + HALF_ULP32 * np.abs(w.imag)))
    r[np.isnan(r)] = np.inf
    return r


def check_clips(got, want, f64, what):
    """every frame of every clip; got / want: per clip -> the worst ratio to the gate"""
    worst, where = 0.0, None
    for c, (g, w) in enumerate(zip(got, want)):
        assert g.shape[0] == w.shape[0], (what, c, g.shape, w.shape)
        if g.size == 0:
            continue
        r = gate_ratio(g, w, f64)
        i = int(np.argmax(r))
        if r.flat[i] > worst:
            worst, where = float(r.flat[i]), (c,) + tuple(int(v) for v in np.unravel_index(i, r.shape))
    assert worst <= 1.0, f"{what}: {worst:.3e} x the gate at (clip, frame, bin) = {where}"
    return worst


def check_mel(got, want, tol, what):
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    d[np.isnan(d)] = np.inf
    i = int(np.argmax(d))
    assert d.flat[i] <= tol, f"{what}: |diff| {float(d.flat[i]):.3e} > {tol:.1e} at (frame, mel) = {tuple(int(v) for v in np.unravel_index(i, d.shape))}"
    return float(d.flat[i]) / tol


def _written(bits, f64, what):
    """(b) no sentinel where a frame belongs.  A double's low word may be any pattern, so complex128 output is read as 64-bit words: two
    sentinel words are a NaN no kernel computes"""
    if f64:
        left = bits.view(np.uint64) == SENTINEL64
        assert not left.any(), f"{what}: {int(left.sum())} doubles never written (first at double {int(np.argmax(left))})"
    else:
        _no_sentinel(bits, what)


def _bits_of(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_mirror(full, what):
    """full layout [..., n_fft]: bin n_fft - k is bit for bit the conjugate of bin k, 0 < k <= (n_fft - 1) / 2 (no Nyquist partner at odd n_fft)"""
    n = full.shape[-1]
    h = (n - 1) // 2
    lo, hi = full[..., 1:h + 1], full[..., n - 1:n - 1 - h:-1]
    assert np.array_equal(_bits_of(lo.real), _bits_of(hi.real)), f"{what}: Re X[n_fft - k] is not Re X[k] bit for bit"
    assert np.array_equal(_bits_of(-lo.imag), _bits_of(hi.imag)), f"{what}: Im X[n_fft - k] is not -Im X[k] bit for bit"


def check_half_is_full(half, full, what):
    b = half.shape[-1]
    assert np.array_equal(_bits_of(half.real), _bits_of(full[..., :b].real)) and np.array_equal(_bits_of(half.imag), _bits_of(full[..., :b].imag)), \
        f"{what}: bins 0 .. n_fft/2 of the full call are not the half call's bit for bit"


# ---- the fenced runners ------------------------------------------------------------------------------------------------------------

def run_uniform(gpu, m, d_pcm, n_clips, n, f64, full):
    nf, bins = m.num_frames(n), m.stft_bins(full)
    out = Fence(gpu, n_clips * nf * bins * WORDS[f64])
    m.stft_uniform_device(d_pcm, n, n, n_clips, out.ptr, f64=f64, full=full)
    m.synchronize()
    bits = out.bits()                                                                          # (a)
    _written(bits, f64, f"uniform {_label(f64, full)}")
    return bits.view(CDT[f64]).reshape(n_clips, nf, bins)


def run_ragged(gpu, m, clips, f64, full):
    """outputs in reverse clip order, a gap of 1 + 2 (c % 4) complex elements in front of every one (offsets in complex elements: complex64
    outputs then start at addresses that are only 8-byte aligned) -> the frames of each clip"""
    lens = [len(x) for x in clips]
    frames = [m.num_frames(n) for n in lens]
    bins, wpc = m.stft_bins(full), WORDS[f64]
    oo, gaps, cur = [0] * len(lens), [], 0
    for c in reversed(range(len(lens))):
        g = 1 + 2 * (c % 4)
        gaps.append((cur, cur + g))
        oo[c] = cur + g
        cur += g + frames[c] * bins
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    pcm, out = _upload(gpu, np.concatenate(clips)), Fence(gpu, cur * wpc)
    m.stft_ragged_device(pcm.ptr, offs, np.array(lens, np.uint64), out.ptr, np.array(oo, np.uint64), f64=f64, full=full)
    m.synchronize()
    bits = out.bits()                                                                          # (a)
    pcm.free()
    for a, b in gaps:                                                                          # (c)
        assert np.all(bits[a * wpc:b * wpc] == SENTINEL), f"ragged {_label(f64, full)}: the gap at complex [{a}, {b}) was written"
    got = []
    for o, f in zip(oo, frames):
        mine = bits[o * wpc:(o + f * bins) * wpc]
        _written(mine, f64, f"ragged {_label(f64, full)}")
        got.append(mine.view(CDT[f64]).reshape(f, bins))
    return got


# ---- 1. whisper400_stft_kernel -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("edge", EDGES)
def test_whisper_stft_uniform_whole_batch(gpu, oracle, edge):
    """(complex128, full) and (complex64, half) on every edge of the partition; all four layouts and the two exact properties on plus1"""
    cus = _cus()
    fft, hop, nm = W400
    n_clips, u, frames = whisper_batch(edge, cus)
    facts = edge_facts("precise", n_clips * u, cus)
    check_edge(edge, facts, u, cus)
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    assert m.uses_fast_path
    n = fft + (frames - 1) * hop
    clips = _noise(n_clips, n, 11000)
    want = stft_ref(oracle, ("w400", edge, cus), clips, fft, hop)
    pcm = _upload(gpu, clips)
    combos = [(True, True), (False, False)] + ([(True, False), (False, True)] if edge == "plus1" else [])
    got, worst = {}, {}
    for f64, full in combos:
        g = run_uniform(gpu, m, pcm.ptr, n_clips, n, f64, full)
        worst[_label(f64, full)] = round(check_clips(list(g), want, f64, f"whisper400 {edge} {_label(f64, full)}"), 6)
        if edge == "plus1":
            got[f64, full] = g
    pcm.free()
    if edge == "plus1":
        for f64 in (True, False):
            check_mirror(got[f64, True], f"whisper400 {_label(f64, True)}")
            check_half_is_full(got[f64, False], got[f64, True], f"whisper400 {'c128' if f64 else 'c64'}")
    print(f"\nSTFT-WHOLE-BATCH whisper400-{edge}: frames={n_clips * frames} worst/gate={worst} {facts}")
    m.close()


@pytest.mark.gpu
def test_whisper_stft_ragged_whole_batch(gpu, oracle):
    cus = _cus()
    fft, hop, nm = W400
    lens = ragged_lengths(fft, hop, 160, fft + 150 * hop, 7)
    base = _noise(len(lens), max(lens), 12000)
    clips = [b[:n] for b, n in zip(base, lens)]
    want = stft_ref(oracle, "w400-ragged", clips, fft, hop)
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    worst = {}
    for f64, full in ((False, False), (True, True)):
        got = run_ragged(gpu, m, clips, f64, full)
        worst[_label(f64, full)] = round(check_clips(got, want, f64, f"whisper400 ragged {_label(f64, full)}"), 6)
    units = sum((m.num_frames(n) + 4) // 5 for n in lens)
    print(f"\nSTFT-WHOLE-BATCH whisper400-ragged: frames={sum(w.shape[0] for w in want)} worst/gate={worst} {edge_facts('precise', units, cus)}")
    m.close()


@pytest.mark.gpu
def test_stft_host_call_is_the_device_call(gpu, oracle):
    """melspec_stft_host on one clip of 30 s into a fenced host array: the device call's bits; a capacity one complex element short is
    MELSPEC_ERR_CAPACITY and leaves the array alone"""
    from mel_spec_amd._lib import lib
    fft, hop, nm = W400
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    x = _noise(1, 30 * 16000, 13000)
    nf = m.num_frames(x.shape[1])
    assert nf == 2998
    want = stft_ref(oracle, "w400-host", x, fft, hop)
    pcm = _upload(gpu, x)
    worst = {}
    for f64, full in ((True, True), (False, False)):
        dev = run_uniform(gpu, m, pcm.ptr, 1, x.shape[1], f64, full)[0]
        bins = m.stft_bins(full)
        words = nf * bins * WORDS[f64]
        host = np.full(words + 2 * HOST_GUARD, SENTINEL, np.uint32)
        body = host[HOST_GUARD:HOST_GUARD + words]
        done = C.c_size_t(0)

        def call(capacity):
            return lib().melspec_stft_host(m._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[1], body.ctypes.data_as(C.c_void_p), capacity,
                                           int(f64), int(full), C.byref(done))
        assert call(nf * bins - 1) == ERR_CAPACITY and done.value == 0
        assert np.all(host == SENTINEL), "a refused host call wrote to its output"
        assert call(nf * bins) == 0 and done.value == nf
        assert np.all(host[:HOST_GUARD] == SENTINEL) and np.all(host[HOST_GUARD + words:] == SENTINEL), "host call: a write outside the output"
        _written(body, f64, f"host {_label(f64, full)}")
        got = body.view(CDT[f64]).reshape(nf, bins)
        assert np.array_equal(_bits_of(got.real), _bits_of(dev.real)) and np.array_equal(_bits_of(got.imag), _bits_of(dev.imag))
        worst[_label(f64, full)] = round(check_clips([got], want, f64, f"host {_label(f64, full)}"), 6)
    pcm.free()
    print(f"\nSTFT-WHOLE-BATCH whisper400-host: frames={nf} worst/gate={worst}")
    m.close()


# ---- 2. generic_stft_kernel --------------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", GENERIC_BATCHES)
@pytest.mark.parametrize("transform", list(GENERIC))
def test_generic_stft_uniform_whole_batch(gpu, oracle, transform, kind):
    """(complex128, full) and (complex64, half) below, at and past the grid cap; all four layouts and the exact properties on cap + 1"""
    cus = _cus()
    fft, hop, nm = GENERIC[transform]
    n_clips, frames = generic_batch(kind, cus)
    check_generic_batch(kind, n_clips * frames, cus)
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    assert not m.uses_fast_path
    n = fft + (frames - 1) * hop
    clips = _noise(n_clips, n, 14000)
    want = stft_ref(oracle, ("generic", kind, cus), clips, fft, hop)
    pcm = _upload(gpu, clips)
    combos = [(True, True), (False, False)] + ([(True, False), (False, True)] if kind == "cap+1" else [])
    got, worst = {}, {}
    for f64, full in combos:
        g = run_uniform(gpu, m, pcm.ptr, n_clips, n, f64, full)
        worst[_label(f64, full)] = round(check_clips(list(g), want, f64, f"generic {transform} {kind} {_label(f64, full)}"), 6)
        if kind == "cap+1":
            got[f64, full] = g
    pcm.free()
    if kind == "cap+1":
        for f64 in (True, False):
            check_mirror(got[f64, True], f"generic {transform} {_label(f64, True)}")
            check_half_is_full(got[f64, False], got[f64, True], f"generic {transform} {'c128' if f64 else 'c64'}")
    print(f"\nSTFT-WHOLE-BATCH generic-{transform}-{kind}: n_fft={fft} clips={n_clips} frames={n_clips * frames} cap={8 * cus} worst/gate={worst}")
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("transform", list(GENERIC))
def test_generic_stft_ragged_whole_batch(gpu, oracle, transform):
    fft, hop, nm = GENERIC[transform]
    rng = np.random.default_rng(15)
    lens = [fft + 17 * hop + 3, fft - 1, 0, fft, fft + hop - 1, fft + 40 * hop, 0, fft + hop] + [int(v) for v in rng.integers(fft, fft + 40 * hop, 9)]
    base = _noise(len(lens), max(lens), 15000)
    clips = [b[:n] for b, n in zip(base, lens)]
    want = stft_ref(oracle, "generic-ragged", clips, fft, hop)
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    assert not m.uses_fast_path
    worst = {}
    for f64, full in ((True, True), (False, False)):
        got = run_ragged(gpu, m, clips, f64, full)
        worst[_label(f64, full)] = round(check_clips(got, want, f64, f"generic {transform} ragged {_label(f64, full)}"), 6)
        if full:
            for g in got:
                check_mirror(g, f"generic {transform} ragged")
    print(f"\nSTFT-WHOLE-BATCH generic-{transform}-ragged: n_fft={fft} frames={sum(w.shape[0] for w in want)} worst/gate={worst}")
    m.close()


# ---- 3. the mel stage past one grid ------------------------------------------------------------------------------------------------

def run_stage(gpu, m, d_spec, n_frames, f64, full):
    out = Fence(gpu, n_frames * m.n_mels)
    m.mel_from_stft_device(d_spec, n_frames, out.ptr, f64=f64, full=full)
    m.synchronize()
    bits = out.bits()                                                                          # (a)
    _no_sentinel(bits, "mel stage")
    return bits.view(np.float32).reshape(n_frames, m.n_mels)


def export_then_stage(gpu, m, x, f64, full):
    """stft_uniform_device of one clip into a fenced device buffer, mel_from_stft_device from there into a fenced [frames][n_mels]"""
    nf, bins = m.num_frames(len(x)), m.stft_bins(full)
    pcm, spec = _upload(gpu, x), Fence(gpu, nf * bins * WORDS[f64])
    m.stft_uniform_device(pcm.ptr, len(x), len(x), 1, spec.ptr, f64=f64, full=full)
    got = run_stage(gpu, m, spec.ptr, nf, f64, full)
    _written(spec.bits(), f64, "the stage's input")
    pcm.free()
    return got


def stage_clip(geo, n_frames, seed):
    fft, hop, _ = geo
    return _noise(1, fft + (n_frames - 1) * hop, seed)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("f64,full", [(True, False), (False, True)], ids=["c128-half", "c64-full"])
@pytest.mark.parametrize("ctx", list(STAGE))
def test_mel_stage_jobs_kernel_past_one_grid(gpu, oracle, ctx, f64, full):
    """F1 = 2 x CUs x 32 + 13 frames: whatever the launcher's workgroups per CU (at most 4, of eight waves), every wave of
    mel_stage_jobs_kernel prefetches and takes at least a second frame, and the last trip is partial; 512 bins: the tail past 256 bins"""
    cus = _cus()
    geo = STAGE[ctx]
    fft, hop, nm = geo
    takes, per_cu, lds = stage_rule(oracle, fft, nm)
    assert takes, (geo, lds)
    F1 = stage_f1(cus)
    step = min(-(-F1 // 8), cus * per_cu) * 8
    assert F1 >= 2 * step and F1 % step != 0
    x = stage_clip(geo, F1, 16000)
    want = mel_ref_long(oracle, "F1", x, fft, hop, nm)
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    got = export_then_stage(gpu, m, x, f64, full)
    worst = check_mel(got, want, MEL_TOL[f64], f"mel stage {geo} {_label(f64, full)}")
    print(f"\nSTFT-WHOLE-BATCH mel-stage-{ctx}-{_label(f64, full)}: frames={F1} waves={step} per_cu={per_cu} lds={lds} worst/gate={worst:.4f}")
    m.close()


@pytest.mark.gpu
def test_mel_stage_small_frame_counts(gpu, oracle):
    """1, 7, 8 and 9 frames: a partial workgroup, a full one, one frame into the second"""
    geo = STAGE["80"]
    fft, hop, nm = geo
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    worst = 0.0
    for nf in (1, 7, 8, 9):
        x = stage_clip(geo, nf, 17000 + nf)
        want = oracle.compute_mel_spectrogram_cpu(x, fft, hop, nm, SR)
        for f64, full in ((True, False), (False, True)):
            got = export_then_stage(gpu, m, x, f64, full)
            worst = max(worst, check_mel(got, want, MEL_TOL[f64], f"mel stage {nf} frames {_label(f64, full)}"))
    print(f"\nSTFT-WHOLE-BATCH mel-stage-small: worst/gate={worst:.4f}")
    m.close()


@pytest.mark.gpu
def test_mel_stage_on_the_oracles_spectra(gpu, oracle):
    """the stage on its own: F1 frames of the ORACLE's half spectra, uploaded"""
    cus = _cus()
    geo = STAGE["80"]
    fft, hop, nm = geo
    F1 = stage_f1(cus)
    x = stage_clip(geo, F1, 16000)
    spec = np.ascontiguousarray(stft_ref_long(oracle, "F1", x, fft, hop)[:, :fft // 2 + 1])
    want = mel_ref_long(oracle, "F1", x, fft, hop, nm)
    m = gpu.HipMelSpectrogram(fft, hop, SR, nm)
    d_spec = _upload(gpu, spec)
    got = run_stage(gpu, m, d_spec.ptr, F1, True, False)
    d_spec.free()
    worst = check_mel(got, want, MEL_TOL[True], "mel stage on the oracle's spectra")
    print(f"\nSTFT-WHOLE-BATCH mel-stage-oracle-spectra: frames={F1} worst/gate={worst:.4f}")
    m.close()


@pytest.mark.gpu
def test_mel_stage_fallback_kernel_past_one_grid(gpu, oracle):
    """more than 256 mels: mel_stage_kernel<T, 4>, at most CUs x 16 workgroups of four waves; F2 = 2 x CUs x 64 + 5 frames of complex64
    half spectra: every wave takes at least two trips of the grid-stride loop"""
    cus = _cus()
    m = None
    for geo in STAGE_FALLBACK:
        try:
            m = gpu.HipMelSpectrogram(geo[0], geo[1], SR, geo[2])
            break
        except gpu.HipUnavailable:
            continue
    assert m is not None
    fft, hop, nm = geo
    assert not stage_rule(oracle, fft, nm)[0]
    F2 = stage_f2(cus)
    step = min(-(-F2 // 4), cus * 16) * 4
    assert F2 >= 2 * step and F2 % step != 0
    x = stage_clip(geo, F2, 18000)
    want = mel_ref_long(oracle, "F2", x, fft, hop, nm)
    got = export_then_stage(gpu, m, x, False, False)
    worst = check_mel(got, want, MEL_TOL[False], f"mel stage fallback {geo}")
    print(f"\nSTFT-WHOLE-BATCH mel-stage-fallback: geometry={geo} frames={F2} waves={step} worst/gate={worst:.4f}")
    m.close()


# ---- 4. streaming spectra, several streams per push --------------------------------------------------------------------------------

def gpu_error():
    from mel_spec_amd._lib import last_error
    return last_error()


def push_stft_fenced(bank, ids, chunks, f64, full):
    """StreamBank.push_stft into a host array with the sentinel either side -> (spectra per stream, frames per stream)"""
    from mel_spec_amd._lib import lib
    a = np.ascontiguousarray(ids, np.uint32)
    lens = np.array([len(c) for c in chunks], np.uint32)
    flat = np.ascontiguousarray(np.concatenate(chunks) if chunks else np.zeros(0), np.float32)
    bins = bank._mel.stft_bins(full)
    cap = sum(bank.frames_after(int(s), int(n)) for s, n in zip(a, lens))
    words = cap * bins * WORDS[f64]
    host = np.full(words + 2 * HOST_GUARD, SENTINEL, np.uint32)
    body = host[HOST_GUARD:HOST_GUARD + words]
    frames = np.zeros(len(ids), np.uint32)
    u32p = C.POINTER(C.c_uint32)
    rc = lib().melspec_stream_push_host_stft(bank._h, a.ctypes.data_as(u32p), flat.ctypes.data_as(C.POINTER(C.c_float)), lens.ctypes.data_as(u32p), len(ids),
                                             body.ctypes.data_as(C.c_void_p), cap * bins, frames.ctypes.data_as(u32p), int(f64), int(full))
    assert rc == 0, (rc, gpu_error())
    assert np.all(host[:HOST_GUARD] == SENTINEL) and np.all(host[HOST_GUARD + words:] == SENTINEL), "push: a write outside the output"
    _written(body, f64, "push")
    out = body.view(CDT[f64]).reshape(cap, bins)
    ends = np.cumsum(frames)
    assert int(frames.sum()) == cap
    return [out[int(e - f):int(e)] for e, f in zip(ends, frames)], [int(f) for f in frames]


@pytest.mark.gpu
@pytest.mark.parametrize("fft,hop,f64,full", STREAM_CASES, ids=lambda v: str(v))
def test_streaming_spectra_several_streams_per_push(gpu, oracle, fft, hop, f64, full):
    """7 streams, a random subset per push, chunk sizes around hop and n_fft: each stream's concatenated output is
    compute_all_cpu(x[off:]), off = ceil(n_fft / hop) hop - n_fft, the counts are frames_after's; after reset([2]) stream 2 starts over
    and its neighbours keep their state"""
    n_streams, max_chunk, total, extra = 7, 1500, 24000, 2000
    m = gpu.HipMelSpectrogram(fft, hop, SR, 80)
    assert m.uses_fast_path if fft == 400 else (fft == 512 or not m.uses_fast_path)     # 400: whisper400_stft_kernel, else generic_stft_kernel
    bank = gpu.StreamBank(m, n_streams, max_chunk)
    src = _noise(n_streams, total + extra, 19000)
    off = -(-fft // hop) * hop - fft
    want = stft_ref(oracle, "stream", [s[off:] for s in src], fft, hop)
    rng = np.random.default_rng(fft + hop)
    sizes = [0, 1, hop - 1, hop, hop + 1, 2 * hop, fft - 1, fft, fft + 1, max_chunk]
    pos, got, live, pushes, widest = [0] * n_streams, [[] for _ in range(n_streams)], set(range(n_streams)), 0, 0
    while live:
        ids = [s for s in sorted(live) if rng.random() < 0.7]
        if not ids:
            continue
        chunks = []
        for s in ids:
            n = int(rng.choice(sizes)) if rng.random() < 0.5 else int(rng.integers(0, max_chunk + 1))
            n = min(n, total - pos[s])
            chunks.append(src[s][pos[s]:pos[s] + n])
            pos[s] += n
        counts = [bank.frames_after(s, len(c)) for s, c in zip(ids, chunks)]
        res, frames = push_stft_fenced(bank, ids, chunks, f64, full)
        assert frames == counts
        pushes += 1
        widest = max(widest, sum(1 for f in frames if f))
        for s, r in zip(ids, res):
            got[s].append(r.copy())
            if pos[s] >= total:
                live.discard(s)
    assert widest >= 4                       # pushes that emit for several streams: a ragged launch over the bank's state buffer
    seen = [sum(len(r) for r in g) for g in got]
    assert seen == [(total - off - fft) // hop + 1] * n_streams, seen
    worst = check_clips([np.concatenate(g) for g in got], [w[:k] for w, k in zip(want, seen)], f64, f"stream {fft}/{hop} {_label(f64, full)}")
    # reset([2]); then the same push to streams 1, 2, 3: stream 2 emits the frames of a fresh stream, 1 and 3 go on where they were
    bank.reset([2])
    tail, ids = [[], [], []], [1, 2, 3]
    for a in range(total, total + extra, 1000):
        res, _ = push_stft_fenced(bank, ids, [src[s][a:a + 1000] for s in ids], f64, full)
        for t, r in zip(tail, res):
            t.append(r.copy())
    tail = [np.concatenate(t) for t in tail]
    fresh = oracle.compute_all_cpu(src[2][total + off:], fft, hop)
    assert tail[1].shape[0] == fresh.shape[0]
    w2 = check_clips([tail[1]], [fresh], f64, "stream 2 after its reset")
    for t, s in ((tail[0], 1), (tail[2], 3)):
        assert t.shape[0] == want[s].shape[0] - seen[s], (s, t.shape, want[s].shape, seen[s])
        w2 = max(w2, check_clips([t], [want[s][seen[s]:]], f64, f"stream {s} next to a reset one"))
    print(f"\nSTFT-WHOLE-BATCH stream-{fft}-{hop}-{_label(f64, full)}: pushes={pushes} most-streams-emitting={widest} frames={sum(seen)} "
          f"worst/gate={worst:.6f} after-reset={w2:.6f}")
    bank.close()
    m.close()


# ---- CPU: the reference against numpy, the batch recipes against the partition ---------------------------------------------------

@pytest.mark.parametrize("fft,hop", PIN_GEOMETRIES, ids=lambda v: str(v))
def test_oracle_stft_is_numpy_fft_of_hann_frames(oracle, fft, hop):
    """oracle.compute_all_cpu against numpy.fft.fft(frames x periodic Hann) on 51 frames of noise, every geometry used above: within
    1e-13 x the frame's 2-norm (measured 7e-17 .. 2e-16: four orders inside the f64 gate it referees)"""
    x = oracle.synth_pcm(3, fft + 50 * hop)
    got = oracle.compute_all_cpu(x, fft, hop)
    hann = 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(fft) / fft))
    frames = np.stack([x[f * hop:f * hop + fft].astype(np.float64) for f in range(51)])
    want = np.fft.fft(frames * hann, axis=1)
    assert got.shape == want.shape == (51, fft)
    norm = np.linalg.norm(want, axis=1)
    assert norm.min() > 0.0
    worst = float((np.abs(got - want).max(axis=1) / norm).max())
    print(f"\nSTFT-WHOLE-BATCH oracle-vs-numpy {fft}/{hop}: worst |diff| / ||frame||_2 = {worst:.2e}")
    assert worst <= 1e-13


def test_stft_whole_batch_recipes_land_on_their_edges(oracle):
    """the sizes the GPU tests pick land where they claim, on 256 and 304 CUs: the `precise` partition of whisper400_stft_kernel, the
    grid cap of generic_stft_kernel, two trips of every wave of the mel stage kernels -- and the restated launcher rule names the stage
    kernel each test claims"""
    for cus in (256, 304):
        for e in EDGES:
            n_clips, u, frames = whisper_batch(e, cus)
            f = edge_facts("precise", n_clips * u, cus)
            check_edge(e, f, u, cus)
            assert partition("precise", n_clips * u, cus)[0] == f["grid"]
            assert (frames % 5 != 0) == (u > 1)                                # the clip's last unit is partial
            if e != "fewer":
                assert f["grid"] == cus
            if e == "inside":
                assert 37 % f["run"] != 0 and f["run"] == 3
        for kind in GENERIC_BATCHES:
            n_clips, frames = generic_batch(kind, cus)
            check_generic_batch(kind, n_clips * frames, cus)
            assert n_clips >= 1 and frames >= 1
        F1, F2 = stage_f1(cus), stage_f2(cus)
        for per_cu in (1, 2, 3, 4):                                            # mel_stage_jobs_kernel: whatever the LDS size allows
            step = min(-(-F1 // 8), cus * per_cu) * 8
            assert F1 >= 2 * step and F1 % step != 0
        step = min(-(-F2 // 4), cus * 16) * 4                                  # mel_stage_kernel<T, 4>
        assert F2 >= 2 * step and F2 % step != 0
    assert stage_f1(256) == 16397

    # the restated launcher rule on the contexts of section 3: the banks of up to 128 mels take mel_stage_jobs_kernel (512 bins: its tail
    # past 256), 300 mels take the fallback
    for geo in STAGE.values():
        takes, per_cu, lds = stage_rule(oracle, geo[0], geo[2])
        assert takes and 1 <= per_cu <= 4 and lds <= 64 * 1024, (geo, lds)
    assert STAGE["512bins"][0] // 2 > 256
    for geo in STAGE_FALLBACK:
        assert not stage_rule(oracle, geo[0], geo[2])[0]
