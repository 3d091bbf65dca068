"""The four-wave kernels of the fused 512-point family -- kKaldiRt4, kStreamRt4, kNemoRt6x4, kWRt6x4 (csrc/fused512_route.hpp) -- on a GPU.
An object lands on them when its table blob leaves no room for eight slices in LDS, and the blob grows with the LENGTH of the filters'
intervals: it is a bank of few, wide filters (1 .. 4 bins at 16 kHz; 1 .. 8, 15, 16 mels for Whisper at n_fft = 512) that runs on four
waves, not one of many narrow ones.  They are not the eight-wave kernels with a smaller launch: a Kaldi object's batches run the
round-robin body, LDS holds four slices behind the largest blobs the family sees, the run-time-length mel loops walk intervals of ~128 bins.

REACH below is the one list of configs: next to each the blob bytes, the waves and the K512 its batches run on.  Nothing observes which
kernel a GPU call ran, so tests/test_reach512.py hands the same list to tests/cpp/reach512_host.cpp -- the library's own decision code on
the host -- and compares.  Every bin count is tested next to its first eight-wave neighbour on the same inputs.

Gates are the suite's, not the kernels': Kaldi 1e-4 (test_gpu_parity.TOL, scaled as test_fbank_variants_and_edges does where use_log_fbank
is off), NeMo 1e-4 (test_gpu_parity.TOL), Whisper at 512 2e-6, and bit equality between two calls of one object.  With one bin a band is a
sum of ~128 terms, which no existing gate was set for: test_references_against_float64_numpy measures, on the CPU, how far the references
are from a float64 numpy restatement of the same config on these clips -- Kaldi 4.8e-7 (CMN off) / 3.8e-6 (CMN on, the f32 left fold of the
mean), NeMo 5.8e-7, all under a tenth of the gate, so the gates stay as they are.  (The oracle's projections sum in f64; what is left is
the rounding of its f32 output at |ln| ~ 16.)"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from test_fbank_stream import FLOOR_ROW, _bits, _drive, _left_fold_means

SR = 16000.0
TOL = 1e-4            # Kaldi fbank and the NeMo frontend against the oracle (test_gpu_parity.TOL)
TOL_W512 = 2e-6       # Whisper at n_fft = 512 (test_fused_512_whisper_flavour)
PCM_F32, PCM_S16, OUT_F32, OUT_F16, OUT_BF16 = 0, 1, 0, 1, 2      # MELSPEC_PCM_* / MELSPEC_OUT_* (melspec_hip.h)
TRIP = 256 * 4 * 4    # frames of one grid trip of a four-wave kernel on an MI355X: 256 CUs x 4 waves x 4 frames

# config (an argument of reach512_host) -> the bytes of its table blob, the waves of its f64 kernels, the kernel of a plain batch, of a
# padded / mel-major / feature-major one, and of the stream bank's pushes
REACH = {
    "kaldi:16000:1": dict(blob=36608, waves=4, plain="kKaldiRt4", layout="kKaldiRt4", stream="kStreamRt4"),
    "kaldi:16000:2": dict(blob=31360, waves=4, plain="kKaldiRt4", layout="kKaldiRt4", stream="kStreamRt4"),
    "kaldi:16000:3": dict(blob=27776, waves=4, plain="kKaldiRt4", layout="kKaldiRt4", stream="kStreamRt4"),
    "kaldi:16000:4": dict(blob=25216, waves=4, plain="kKaldiRt4", layout="kKaldiRt4", stream="kStreamRt4"),
    "kaldi:16000:5": dict(blob=23424, waves=8, plain="kKaldiRtRuns", layout="kKaldiRt", stream="kStreamRt"),
    "nemo:16000:1": dict(blob=37120, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "nemo:16000:2": dict(blob=32384, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "nemo:16000:3": dict(blob=28928, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "nemo:16000:4": dict(blob=26496, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "nemo:16000:5": dict(blob=24448, waves=8, plain="kNemoRt6", layout="kNemoRt6", stream="kNone", lds=163776),     # the fullest launch the family makes
    # a blob of exactly 24 576 bytes: eight slices fit, eight slices and the RoundSync counters do not
    "nemo:9600:4": dict(blob=24576, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "nemo:5750:3": dict(blob=24576, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "nemo:4850:3:htk": dict(blob=24576, waves=4, plain="kNemoRt6x4", layout="kNemoRt6x4", stream="kNone"),
    "whisper:16000:1": dict(blob=37120, waves=4, plain="kWRt6x4", layout="kWRt6x4", stream="kNone"),
    "whisper:16000:8": dict(blob=20864, waves=4, plain="kWRt6x4", layout="kWRt6x4", stream="kNone"),
    "whisper:16000:9": dict(blob=19968, waves=8, plain="kWRt6Runs", layout="kWRt6", stream="kNone"),
    "whisper:16000:14": dict(blob=17408, waves=8, plain="kWRt6Runs", layout="kWRt6", stream="kNone"),
    "whisper:16000:15": dict(blob=22656, waves=4, plain="kWRt6x4", layout="kWRt6x4", stream="kNone"),
    "whisper:16000:16": dict(blob=21376, waves=4, plain="kWRt6x4", layout="kWRt6x4", stream="kNone"),
    "whisper:16000:17": dict(blob=20224, waves=8, plain="kWRt6Runs", layout="kWRt6", stream="kNone"),
    "whisper:8000:6": dict(blob=20864, waves=4, plain="kWRt6x4", layout="kWRt6x4", stream="kNone"),
    "whisper:8000:8": dict(blob=18944, waves=8, plain="kWRt6Runs", layout="kWRt6", stream="kNone"),
    # many narrow filters: a small blob, eight waves, ten slots (test_ragged_batch_with_the_clip_table_in_device_memory[512-160-140-auto])
    "whisper:16000:140": dict(blob=14720, waves=8, plain="kWRt10Runs", layout="kWRt10", stream="kNone"),
}
KALDI_BINS = [1, 4, 5]                         # 5: the eight-wave neighbour (kKaldiRtRuns, one slot)
NEMO_MELS = [1, 4, 5]                          # 5: the full-LDS eight-wave neighbour (kNemoRt6)
NEMO_HOLES = [(9600, 4), (5750, 3)]
W512 = [(160, 8, 16000.0), (160, 1, 16000.0), (160, 16, 16000.0), (200, 6, 8000.0), (160, 9, 16000.0)]      # (160, 9): the eight-wave neighbour
assert all(f"kaldi:16000:{b}" in REACH for b in KALDI_BINS) and all(f"nemo:16000:{m}" in REACH for m in NEMO_MELS)
assert all(f"nemo:{sr}:{m}" in REACH for sr, m in NEMO_HOLES) and all(f"whisper:{int(sr)}:{m}" in REACH for _, m, sr in W512)


# ---- inputs and references, computed once ---------------------------------------------------------------------------------------------

_CACHE = {}


def _pmap(fn, items):
    with ThreadPoolExecutor(16) as ex:
        return list(ex.map(fn, items))


def ragged_clips(oracle, jfk):
    """77 clips of at most 1 s, jfk slices and hash noise in turn: empty and sub-frame clips, 3 / 4 / 5 and 7 / 8 / 9 frames of the Kaldi
    geometry (4k - 1, 4k, 4k + 1: a unit is 4 frames), the 511 / 512 samples of the n_fft = 512 contexts, and 62 clips of 14 000 .. 16 000
    samples -- more than one grid trip of a four-wave kernel in every geometry here"""
    if "clips" not in _CACHE:
        rng = np.random.default_rng(4)
        lens = [0, 1, 399, 400, 511, 512, 559, 560, 400 + 2 * 160, 400 + 3 * 160 - 1, 400 + 3 * 160, 400 + 4 * 160, 400 + 6 * 160,
                400 + 7 * 160, 400 + 8 * 160] + [int(v) for v in rng.integers(14000, 16001, 62)]
        lens = [lens[i] for i in rng.permutation(len(lens))]
        _CACHE["clips"] = [np.ascontiguousarray(jfk[(i * 2311) % 150000:][:n]) if i % 2 else oracle.synth_pcm(i, n) for i, n in enumerate(lens)]
    return _CACHE["clips"]


def ragged_ref(key, oracle, jfk, fn):
    """the oracle on every clip of the ragged batch, once per config"""
    if key not in _CACHE:
        _CACHE[key] = _pmap(fn, ragged_clips(oracle, jfk))
    return _CACHE[key]


def _frac(got, want, tol):
    """the worst |got - want| as a fraction of its bound (a NaN counts as infinitely far)"""
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    d[np.isnan(d)] = np.inf
    return float(d.max()) / tol


def _kaldi_cfg(oracle, bins, kw):
    oc = oracle.fbank_default_config()
    oc.num_mel_bins = bins
    for k, v in kw.items():
        setattr(oc, k, int(v) if isinstance(v, bool) else v)
    return oc


def _kaldi_tol(kw, want):
    return TOL if kw.get("use_log_fbank", True) else 1e-4 * max(1.0, float(np.abs(want).max()) if want.size else 1.0)


def _nemo_cfg(oracle, kw):
    return oracle.blm_default_config(**{k: (int(v) if isinstance(v, bool) else v) for k, v in kw.items()})


def _nemo_norm_fracs(oracle, got, raw_gpu, want, raw_want, valid):
    """test_gpu_parity._check_nemo_normalised's two gates as fractions: every row against the reference's literal f32 folds applied to
    the device's own un-normalised rows (2e-5 of max(1, |out|)), and the rows whose std is at least 0.5 against the oracle end to end
    (TOL of max(1, |z|))"""
    lit = oracle.blm_normalize(raw_gpu, valid)
    a = float((np.abs(got - lit) / np.maximum(1.0, np.abs(lit))).max()) / 2e-5 if got.size else 0.0
    std = raw_want[:, :valid].astype(np.float64).std(axis=1, ddof=1) if valid > 1 else np.zeros(raw_want.shape[0])
    good = std >= 0.5
    b = float((np.abs(got[good] - want[good]) / np.maximum(1.0, np.abs(want[good]))).max()) / TOL if good.any() and got.size else 0.0
    return a, b


# ---- the references against float64 numpy (CPU) -------------------------------------------------------------------------------------

def kaldi_f64(oracle, x, bins, apply_cmn):
    """Fbank::compute (src/fbank.rs:141-236) in float64 numpy: default config, `bins` mel bins"""
    x = np.asarray(x, np.float64)
    if len(x) < 400:
        return np.zeros((0, bins))
    nf = 1 + (len(x) - 400) // 160
    idx = np.arange(400)[None, :] + 160 * np.arange(nf)[:, None]
    fr = x[idx]
    mean = fr.mean(axis=1, keepdims=True)
    y = fr - mean
    prev = np.zeros_like(y)
    prev[:, 1:] = y[:, :-1]
    prev[1:, 0] = x[idx[1:, 0] - 1] - mean[1:, 0]             # frame 0 of a clip has no sample in front of it
    y = y - 0.97 * prev
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(400) / 399.0)) ** 0.85
    spec = np.fft.rfft(y * w, 512, axis=1)
    e = (spec.real ** 2 + spec.imag ** 2) @ oracle.kaldi_mel_filterbank(16000.0, 512, bins, 20.0, 8000.0).T
    out = np.log(np.maximum(e, float(np.finfo(np.float32).eps)))
    return out - out.mean(axis=0) if apply_cmn else out


def nemo_f64(oracle, x, n_mels, cols, valid):
    """BatchLogMelSpectrogram::compute (src/mel.rs:299-385) in float64 numpy behind the reference's f32 inputs (pre-emphasised samples,
    window, weights): 16 kHz, centred, pre-emphasis 0.97, no normalisation; cols / valid: the geometry of the output"""
    x = np.asarray(x, np.float32)
    if len(x) == 0:
        return np.zeros((n_mels, cols))
    wave = x.copy()
    wave[1:] = x[1:] - np.float32(0.97) * x[:-1]
    buf = np.zeros(256 + len(x) + 512 + 160 * valid)
    buf[256:256 + len(x)] = wave
    win = np.zeros(512)
    i = np.arange(400, dtype=np.float32)
    win[56:456] = np.float32(0.5) - np.float32(0.5) * np.cos((np.float32(2.0) * np.float32(np.pi) * i) / np.float32(399.0))
    fr = buf[np.arange(512)[None, :] + 160 * np.arange(valid)[:, None]]
    spec = np.fft.rfft(fr * win, axis=1)
    wts = oracle.mel_filterbank(16000.0, 512, n_mels, None, 8000.0).astype(np.float32).astype(np.float64)
    out = np.zeros((n_mels, cols))
    out[:, :valid] = np.log((spec.real ** 2 + spec.imag ** 2) @ wts.T + float(np.finfo(np.float32).eps)).T
    return out


@pytest.mark.parametrize("bins", [1, 4])
def test_references_against_float64_numpy(oracle, jfk, bins):
    """How far the references of the Kaldi and NeMo tests below are from a float64 numpy restatement of the same config, on the tests'
    own clips (the single clips and the whole ragged batch), with 1 and 4 bins.  Measured: Kaldi 4.8e-7 without CMN (1 and 4 bins) and 3.8e-6 / 2.6e-6
    with it, NeMo 4.8e-7 / 5.8e-7 -- under a tenth of the 1e-4 gate, so the gate stays at the suite's value.  (Had it been more, the gate would have been the
    suite's value plus twice the measured distance.)"""
    clips = list(ragged_clips(oracle, jfk)) + [jfk[30000:38000], oracle.synth_pcm(4, 8000), oracle.synth_pcm(2, 16007)]
    worst = {}
    for cmn in (False, True):
        oc = _kaldi_cfg(oracle, bins, dict(apply_cmn=cmn))
        worst[f"kaldi cmn={int(cmn)}"] = max(_frac(oracle.fbank_compute(x, oc), kaldi_f64(oracle, x, bins, cmn), 1.0) for x in clips)
    cfg = _nemo_cfg(oracle, dict(n_mels=bins, preemphasis=0.97))
    d = 0.0
    for x in clips:
        want, valid = oracle.blm_compute(x, cfg, True)
        d = max(d, _frac(want, nemo_f64(oracle, x, bins, want.shape[1], valid), 1.0))
    worst["nemo"] = d
    print(f"{bins} bins: the references' distance from float64 numpy " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert max(worst.values()) < TOL / 10, worst


# ---- Kaldi fbank: kKaldiRt4 -------------------------------------------------------------------------------------------------------------

KALDI_LENS = (0, 399, 400, 559, 560, 400 + 3 * 160 - 1, 400 + 3 * 160, 400 + 4 * 160, 8000)


def _fbank(gpu, bins, **kw):
    fb = gpu.Fbank(gpu.FbankConfig(num_mel_bins=bins, **kw))
    assert fb.uses_fast_path
    return fb


@pytest.mark.gpu
@pytest.mark.parametrize("bins", KALDI_BINS)
def test_kaldi_single_clips(gpu, oracle, jfk, bins):
    """one clip through compute, hash noise and speech, at every length around the four-frame unit: apply_cmn off and on, use_log_fbank off"""
    worst = 0.0
    for kw in (dict(apply_cmn=False), dict(apply_cmn=True), dict(apply_cmn=False, use_log_fbank=False)):
        fb, oc = _fbank(gpu, bins, **kw), _kaldi_cfg(oracle, bins, kw)
        for n in KALDI_LENS:
            for x in (oracle.synth_pcm(4, n), jfk[30000:30000 + n]):
                got, want = fb.compute(x), oracle.fbank_compute(x, oc)
                assert got.shape == (0 if n < 400 else 1 + (n - 400) // 160, bins)
                worst = max(worst, _frac(got, want, _kaldi_tol(kw, want)))
        fb.close()
    print(f"kaldi {bins} bins, single clips: {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("cmn", [False, True], ids=["raw", "cmn"])
@pytest.mark.parametrize("bins", KALDI_BINS)
def test_kaldi_ragged_batch_past_one_grid_trip(gpu, oracle, jfk, bins, cmn):
    """compute_ragged over the 77 clips, more frames than one trip of the four-wave grid: every row of every clip against the oracle
    (with apply_cmn the two-kernel path: four waves are never clip-kernel eligible, and 1 and 5 are no multiples of 4)"""
    clips = ragged_clips(oracle, jfk)
    fb, oc = _fbank(gpu, bins, apply_cmn=cmn), _kaldi_cfg(oracle, bins, dict(apply_cmn=cmn))
    want = ragged_ref(f"kaldi-{bins}-{int(cmn)}", oracle, jfk, lambda x: oracle.fbank_compute(x, oc))
    assert sum(w.shape[0] for w in want) > TRIP
    got = fb.compute_ragged(clips)
    worst = max(_frac(g, w, TOL) for g, w in zip(got, want))
    print(f"kaldi {bins} bins, cmn {int(cmn)}, {sum(w.shape[0] for w in want)} frames in {len(clips)} clips: {worst:.3f} of the bound")
    assert worst <= 1.0
    fb.close()


def _ragged_desc(gpu, obj, clips, nm, slack):
    """compute_ragged_device_desc: the clip table in device memory, packed outputs, max_total_frames = the truth + slack"""
    lens = np.array([len(c) for c in clips], np.uint64)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    frames = [obj.num_frames(int(n)) for n in lens]
    total = sum(frames)
    flat = np.concatenate(clips)
    bufs = [gpu.DeviceBuffer(flat.nbytes), gpu.DeviceBuffer(offs.nbytes), gpu.DeviceBuffer(lens.nbytes), gpu.DeviceBuffer((total + slack) * nm * 4)]
    bufs[0].upload(flat); bufs[1].upload(offs.view(np.float32)); bufs[2].upload(lens.view(np.float32))
    obj.compute_ragged_device_desc(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, len(clips), bufs[3].ptr, 0, total + slack)
    obj.synchronize()
    out = bufs[3].download((total * nm,))
    for b in bufs:
        b.free()
    res, cur = [], 0
    for f in frames:
        res.append(out[cur:cur + f * nm].reshape(f, nm))
        cur += f * nm
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("bins", KALDI_BINS)
def test_kaldi_rows_do_not_depend_on_the_batch(gpu, oracle, jfk, bins):
    """One object, one clip: compute, compute_ragged, compute_uniform_device and compute_ragged_device_desc (the clip table in device
    memory, a tight and a generous frame bound) give the same bits -- without CMN and, through the two-kernel path, with it.  use_generic
    stays within the gate of the oracle and switching back restores the first bits.  No 16-bit kernels for such an object."""
    x, y, z = jfk[50000:58000], oracle.synth_pcm(7, 8000), jfk[90000:98000]
    others = [oracle.synth_pcm(8, 1234), np.zeros(0, np.float32), jfk[1000:1879]]
    worst = 0.0
    for cmn in (False, True):
        fb, oc = _fbank(gpu, bins, apply_cmn=cmn), _kaldi_cfg(oracle, bins, dict(apply_cmn=cmn))
        solo, want = fb.compute(x), oracle.fbank_compute(x, oc)
        worst = max(worst, _frac(solo, want, TOL))
        ragged = fb.compute_ragged(others[:2] + [x] + others[2:])
        assert np.array_equal(_bits(ragged[2]), _bits(solo)), (cmn, "compute_ragged")
        batch = fb.compute_batch(np.stack([y, z, x, y, z, y, x]))
        assert np.array_equal(_bits(batch[2]), _bits(solo)) and np.array_equal(_bits(batch[6]), _bits(solo)), (cmn, "compute_uniform_device")
        for slack in (0, 5000):
            desc = _ragged_desc(gpu, fb, [others[0], x, others[2]], bins, slack)
            assert np.array_equal(_bits(desc[1]), _bits(solo)), (cmn, "compute_ragged_device_desc", slack)
            assert np.array_equal(_bits(desc[2]), _bits(ragged[3]))
        fb.use_generic(True)
        assert not fb.uses_fast_path
        worst = max(worst, _frac(fb.compute(x), want, TOL))
        fb.use_generic(False)
        assert fb.uses_fast_path and np.array_equal(_bits(fb.compute(x)), _bits(solo)), (cmn, "back from the generic kernel")
        for pcm, out in ((PCM_F32, OUT_F16), (PCM_F32, OUT_BF16), (PCM_S16, OUT_F32),
                         (PCM_S16, OUT_F16), (PCM_S16, OUT_BF16)):
            assert not fb.supports_io(pcm, out), (bins, pcm, out)
        fb.close()
    print(f"kaldi {bins} bins, one clip through every entry point + the generic kernel: {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("bins", KALDI_BINS)
def test_kaldi_stream_bank(gpu, oracle, jfk, bins):
    """kStreamRt4: test_fbank_stream's random cuts on 5 streams x 8000 samples, two seeds: rows bit-equal to the batch call of the
    apply_cmn = False twin and between the cuts, means bit-equal to the f64 left fold of the rows, rows within the gate of the oracle"""
    src = [np.ascontiguousarray(jfk[(7919 * s) % 60000:][:8000] * np.float32(1.0 + 0.1 * s)) for s in range(5)]
    fb, twin = _fbank(gpu, bins, apply_cmn=True), _fbank(gpu, bins, apply_cmn=False)
    oc = _kaldi_cfg(oracle, bins, dict(apply_cmn=False))
    runs = []
    for seed in (11, 12):
        bank = gpu.FbankStreamBank(fb, len(src), 1000)
        rows = _drive(bank, src, 160, 1000, seed)
        means, counts = bank.stats(list(range(len(src))))
        bank.close()
        runs.append((rows, means, counts))
    worst = 0.0
    for s in range(len(src)):
        (r1, m1, c1), (r2, m2, _) = runs
        batch, want = twin.compute(src[s]), oracle.fbank_compute(src[s], oc)
        assert r1[s].shape == batch.shape == want.shape and int(c1[s]) == want.shape[0]
        assert np.array_equal(_bits(r1[s]), _bits(batch)), (s, "rows differ from the batch call")
        assert np.array_equal(_bits(r1[s]), _bits(r2[s])) and np.array_equal(_bits(m1[s]), _bits(m2[s])), (s, "another cut, other bits")
        assert np.array_equal(_bits(m1[s]), _bits(_left_fold_means(r1[s]))), (s, "means are not the left fold of the rows")
        worst = max(worst, _frac(r1[s], want, TOL))
    print(f"kaldi {bins} bins, stream bank: rows {worst:.3f} of the bound")
    assert worst <= 1.0
    fb.close(); twin.close()


@pytest.mark.gpu
def test_kaldi_stream_bank_predecessor_sample_at_four_bins(gpu, oracle, jfk):
    """test_fbank_stream.test_gpu_predecessor_sample on kStreamRt4: a NaN at sample shift - 1, pushed as 400 + 160 + 160, is the predecessor
    of the second push's first frame and has to floor it like the reference does; frame 2 does not see it"""
    fb = _fbank(gpu, 4)
    oc = _kaldi_cfg(oracle, 4, dict(apply_cmn=False))
    clean = np.ascontiguousarray(jfk[20000:20720])
    bad = clean.copy(); bad[159] = np.nan
    bank = gpu.FbankStreamBank(fb, 2, 400)
    got = [[], []]
    for lo, hi in ((0, 400), (400, 560), (560, 720)):
        a, b = bank.push([0, 1], [clean[lo:hi], bad[lo:hi]])
        got[0].append(a.copy()); got[1].append(b.copy())
    c, p = np.concatenate(got[0]), np.concatenate(got[1])
    want = oracle.fbank_compute(bad, oc)
    assert c.shape == p.shape == want.shape == (3, 4)
    ulps4 = 4 * 2.0 ** -20
    assert np.abs(want[:2] - FLOOR_ROW).max() <= ulps4
    assert np.isfinite(p).all() and np.abs(p[:2] - FLOOR_ROW).max() <= ulps4, "the predecessor of a push's first frame did not reach it"
    worst = _frac(c, oracle.fbank_compute(clean, oc), TOL)
    assert np.array_equal(_bits(p[2]), _bits(c[2])) and worst <= 1.0
    print(f"kaldi 4 bins, predecessor sample: clean rows {worst:.3f} of the bound")
    bank.close(); fb.close()


# ---- NeMo frontend: kNemoRt6x4 -----------------------------------------------------------------------------------------------------------

def _nemo(gpu, **kw):
    return gpu.BatchLogMelSpectrogram(gpu.BatchLogMelConfig(**kw))


def _no_16bit_no_split(gpu, fe):
    assert not fe.supports_split()
    for pcm in (PCM_F32, PCM_S16):
        for out in (OUT_F32, OUT_F16, OUT_BF16):
            if (pcm, out) != (PCM_F32, OUT_F32):
                assert not fe.supports_io(pcm, out), (pcm, out)


def _nemo_single(gpu, oracle, kw, clips):
    """compute on each clip against the oracle -> the worst fraction; with normalize_per_feature the two gates of _nemo_norm_fracs"""
    fe, cfg = _nemo(gpu, **kw), _nemo_cfg(oracle, kw)
    raw_kw = dict(kw, normalize_per_feature=False)
    raw_fe, raw_cfg = _nemo(gpu, **raw_kw), _nemo_cfg(oracle, raw_kw)
    worst = 0.0
    for x in clips:
        got = fe.compute(x)
        want, valid = oracle.blm_compute(x, cfg, True)
        assert got.shape == want.shape and fe.num_frames(len(x)) == valid
        if not want.size:
            continue
        if kw.get("normalize_per_feature"):
            raw, (raw_want, _) = raw_fe.compute(x), oracle.blm_compute(x, raw_cfg, True)
            worst = max(worst, _frac(raw, raw_want, TOL), *_nemo_norm_fracs(oracle, got, raw, want, raw_want, valid))
        else:
            worst = max(worst, _frac(got, want, TOL))
    fe.close(); raw_fe.close()
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", NEMO_MELS)
def test_nemo_single_clips(gpu, oracle, jfk, n_mels):
    """compute with pre-emphasis 0.97: normalize_per_feature off and on, pad_to 0 and 16, centred or not; no split output, no 16-bit kernels"""
    clips = [jfk[20000:28000], oracle.synth_pcm(2, 16007), oracle.synth_pcm(4, 300), oracle.synth_pcm(5, 512 + 3 * 160), np.zeros(0, np.float32)]
    worst = 0.0
    for norm in (False, True):
        for pad_to in (0, 16):
            for center in (True, False):
                worst = max(worst, _nemo_single(gpu, oracle, dict(n_mels=n_mels, preemphasis=0.97, normalize_per_feature=norm, pad_to=pad_to, center=center), clips))
    fe = _nemo(gpu, n_mels=n_mels, preemphasis=0.97)
    _no_16bit_no_split(gpu, fe)
    fe.close()
    print(f"nemo {n_mels} mels, single clips: {worst:.3f} of the bound")
    assert worst <= 1.0


def _nemo_ragged(gpu, oracle, jfk, key, kw, clips=None):
    """compute_ragged, normalisation off and on, every clip against the oracle -> the worst fraction"""
    clips = ragged_clips(oracle, jfk) if clips is None else clips
    worst, raw, raw_want = 0.0, None, None
    for norm in (False, True):
        kwn = dict(kw, normalize_per_feature=norm)
        fe, cfg = _nemo(gpu, **kwn), _nemo_cfg(oracle, kwn)
        fn = lambda x: oracle.blm_compute(x, cfg, True)
        want = ragged_ref(f"{key}-{int(norm)}", oracle, jfk, fn) if clips is ragged_clips(oracle, jfk) else _pmap(fn, clips)
        got = fe.compute_ragged(clips)
        fe.close()
        if not norm:
            raw, raw_want = got, want
            worst = max(worst, max(_frac(g, w, TOL) for g, (w, _) in zip(got, want)))
        else:
            for g, r, (w, valid), (rw, _) in zip(got, raw, want, raw_want):
                assert g.shape == w.shape
                if w.size:
                    worst = max(worst, *_nemo_norm_fracs(oracle, g, r, w, rw, valid))
    return worst, sum(v for _, v in raw_want)


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", NEMO_MELS)
def test_nemo_ragged_batch_past_one_grid_trip(gpu, oracle, jfk, n_mels):
    worst, frames = _nemo_ragged(gpu, oracle, jfk, f"nemo-{n_mels}", dict(n_mels=n_mels, preemphasis=0.97))
    assert frames > TRIP
    print(f"nemo {n_mels} mels, {frames} frames, normalisation off and on: {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", NEMO_MELS)
def test_nemo_uniform_device(gpu, oracle, n_mels):
    """compute_uniform_device: 33 clips of 4 * 160 * 5 + 1 samples (the last unit of every clip holds one frame)"""
    kw = dict(n_mels=n_mels, preemphasis=0.97)
    clips = np.stack([oracle.synth_pcm(100 + c, 4 * 160 * 5 + 1) for c in range(33)])
    fe, cfg = _nemo(gpu, **kw), _nemo_cfg(oracle, kw)
    got = fe.compute_batch(clips)
    want = _pmap(lambda x: oracle.blm_compute(x, cfg, True)[0], list(clips))
    worst = max(_frac(g, w, TOL) for g, w in zip(got, want))
    fe.close()
    print(f"nemo {n_mels} mels, 33 equal clips: {worst:.3f} of the bound")
    assert worst <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("sr,n_mels", NEMO_HOLES)
def test_nemo_blob_of_exactly_24576_bytes(gpu, oracle, jfk, sr, n_mels):
    """The table blob of these banks is exactly 24 576 bytes: eight slices fit beside it, eight slices and the RoundSync counters do not.
    The create call used to ask the 8-or-4 question without the counters and dropped such an object off the fused path; it now runs on
    four waves (tests/test_reach512.py).  The rows were right on either path: a single clip and a ragged batch against the oracle."""
    kw = dict(sample_rate=sr, n_mels=n_mels, preemphasis=0.97)
    worst = _nemo_single(gpu, oracle, kw, [jfk[20000:28000], oracle.synth_pcm(2, 16007)])
    worst = max(worst, _nemo_ragged(gpu, oracle, jfk, "", kw, ragged_clips(oracle, jfk)[:24])[0])
    fe = _nemo(gpu, **kw)
    _no_16bit_no_split(gpu, fe)
    fe.close()
    print(f"nemo {sr} Hz {n_mels} mels: {worst:.3f} of the bound")
    assert worst <= 1.0


# ---- Whisper at n_fft = 512: kWRt6x4 -----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("hop,n_mels,sr", W512, ids=lambda v: str(int(v)))
def test_whisper_512(gpu, oracle, jfk, hop, n_mels, sr):
    """test_fused_512_whisper_flavour's body on the few-mel banks: single clips incl. 0 / 511 / 512 samples, a 21-clip batch, a ragged batch
    with an empty clip, the four interleaved layouts; then a ragged batch past one grid trip, every clip against the oracle, and a
    StreamBank of 3 streams fed hop by hop, bit-equal to the one-shot call on the stream's samples"""
    m = gpu.HipMelSpectrogram(512, hop, sr, n_mels)
    assert m.uses_fast_path and "n_fft = 512, f64" in m.plain_kernel_name()
    ref = lambda y: oracle.compute_mel_spectrogram_cpu(y, 512, hop, n_mels, sr)
    x = jfk[20000:61000]
    worst = _frac(m.compute_mel_spectrogram(x), ref(x), TOL_W512)
    for n in (0, 511, 512, 512 + 3 * hop, 512 + 4 * hop + 7):
        y = oracle.synth_pcm(5, n)
        worst = max(worst, _frac(m.compute_mel_spectrogram(y), ref(y), TOL_W512))
    clips = np.stack([oracle.synth_pcm(c, 8000) for c in range(21)])
    b = m.compute_batch(clips)
    worst = max(worst, max(_frac(b[c], ref(clips[c]), TOL_W512) for c in range(21)))
    srcs = (jfk[:3000], np.zeros(0, np.float32), jfk[100:700], jfk[5:9000])
    worst = max(worst, max(_frac(r, ref(s), TOL_W512) for r, s in zip(m.compute_ragged(list(srcs)), srcs)))
    for major, min_width in ((False, 0), (False, 100), (True, 2), (True, 64)):
        il = m.compute_batch_interleaved(clips[:3], major, min_width)
        for c in range(3):
            worst = max(worst, _frac(il[c], oracle.interleave_frames(ref(clips[c]), major, min_width), TOL_W512))
    # past one grid trip
    rag = ragged_clips(oracle, jfk)
    want = ragged_ref(f"w512-{hop}-{n_mels}-{int(sr)}", oracle, jfk, ref)
    frames = sum(w.shape[0] for w in want)
    assert frames > TRIP
    worst = max(worst, max(_frac(g, w, TOL_W512) for g, w in zip(m.compute_ragged(rag), want)))
    # the stream bank: hop-sized pushes, the rows of samples[off:]'s frames (off = ceil(n_fft / hop) * hop - n_fft)
    pushes, off = 60, -(-512 // hop) * hop - 512
    src = [np.ascontiguousarray(jfk[40000 + 5000 * s:][:pushes * hop] * np.float32(1.0 + 0.1 * s)) for s in range(3)]
    bank = gpu.StreamBank(m, 3, hop)
    rows = [[] for _ in src]
    for k in range(pushes):
        for s, r in enumerate(bank.push([0, 1, 2], [v[k * hop:(k + 1) * hop] for v in src])):
            rows[s].append(r.copy())
    bank.close()
    for s, v in enumerate(src):
        one = m.compute_mel_spectrogram(v[off:])
        got = np.concatenate(rows[s])
        assert got.shape == one.shape == (pushes - (-(-512 // hop) - 1), n_mels)
        assert np.array_equal(_bits(got), _bits(one)), (s, "the stream's rows differ from the one-shot call")
    print(f"whisper 512 / {hop} / {n_mels} mels / {int(sr)} Hz, {frames} ragged frames: {worst:.3f} of the bound")
    assert worst <= 1.0
    m.close()
