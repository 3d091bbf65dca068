"""The raw rows of the centred Whisper features (melspec_whisper_*_split) gated on their mean error and on their per-band and per-slot
bias, not only on their largest error -- tests/test_f32_statistics.py and tests/test_f64_statistics.py for the kernels that came after
them: the raw epilogue (six_raw_store: biased value - 16), the f64 kernel on gathered edge frames through a hand-built batch, the
slot_map indirection and wc_clip_max_kernel.  tests/test_whisper_centered.py bounds the largest difference only (8e-6 raw in F64, 6e-4
normalised in F32, where the last measurement had 5.7e-7 and 4.2e-6 normalised); nothing is clamped in the split call's rows, so the
statistic is taken on every value (clamp=False throughout).

Machinery: err_stats / gate_failures / report / MARGIN of tests/test_f32_statistics.py and log_allowance / stats64 / check64 of
tests/test_f64_statistics.py, as they stand.  Reference: whisper_centered_ref.raw_rows_many (f64).  Nothing is committed as a constant.

Inputs, Gaussian noise at 0.1 from np.random.default_rng(64) in this order, all at pad_to = 0:
    long    40 clips of 16 037 samples: T = 100, frames 0, 1 and 99 are edge frames, 2 .. 98 interior
    short   600 clips of 1000 + (37 i) % 160 samples: T = 6 with edge frames 0 and 1 (n < 1120) or T = 7 with edge frames 0, 1 and 6 --
            1 347 edge frames in all (at pad_to = 0 a clip has at most four; five -- kWcMaxEdges -- take a pad_to: the row below)
and one row more than the rows at pad_to = 0: `short` at pad_to = 1600 (T = 10: edge frames 0, 1, 6, 7 and, from 1081 samples, 8 -- the
frames that straddle the end of the samples, which pad_to = 0 never has -- and one or two silent frames, which must be exactly -10).

Yardsticks, with the kernels' declared ending: the kernels carry log10 E + 16 as one float32 in [6, ~30] and store it minus 16, so a raw
row honestly carries half an ulp at magnitude 8 - 32 (up to 0.95e-6).  F64: the f64 energies -> float32 -> float32 log10 -> + 16 rounded to
float32 -> max(., 6) -> - 16.  F32: the same ending on whisper_f32's float32 energies of the reflect-padded signal.  Allowance for the
hardware log: log_allowance(E, log10(2)), the Whisper allowance of tests/test_f64_statistics.py without the division by 4.

Slots.  Interior frame t is frame t - 2 of the interior's batch: its slot is (t - 2) mod 6, the frame's place in the six-frame unit.
An edge frame's slot is its position among its clip's edge frames (period 5 = kWcMaxEdges); in a row over all frames the edge frames
join the slots of the same number.

Every GPU row also asserts that the returned clip maximum is, bit for bit, the float32 maximum of the clip's returned rows: both are
`biased - 16.0f` of the same bits, so a flush to the wrong word, a flush lost at a run's end or a wrong slot_map entry breaks it.

Measured on the device (profiles/whisper_centered_stats.txt): every row x 1.77 - 2.05 of its yardstick before the allowance, x 0.48 - 1.17
after it -- the offset every band and slot share (-1.4e-7 against the yardstick's -7.8e-8) is v_log_f32's, inside L.  No row has a margin
of its own.  Once, in a scratch build (not committed): 16.0f in six_raw_store replaced by the next float32 above it -- every row went red
(mean x 7.1 - 7.6, band bias x 14 - 20, slot bias x 10 - 30 after L; largest error 4.1e-6 in F64, under the 8e-6 gate) and so did the
maximum's bit equality, while the 38 GPU cases tests/test_whisper_centered.py had before stayed green.

The third perturbation of the CPU test (one Hann tap x (1 + 1e-3), edge frames) is red on the band bias by x 560, but it is NOT under the
old maximum gate: a tap moves single bins, and a low band of one or two bins whose bin happens to be small (|X|^2 is exponentially
distributed) moves by far more than its mean -- measured 4.0e-2 at tap 57, and 1.1e-4 still at tap 3, against the gate of 8e-6.  No tap
of the first 200 stays under it and is seen (checked at taps 3, 10, 20, 40, 57, 100, 150, 199), so the test asserts `under the old gate`
for the band and for the subtrahend only, like tests/test_f32_statistics.py does for its tap."""
import functools

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_whole_batch.py)  # noqa: F401

import whisper_centered_ref as R
from test_f32_statistics import MARGIN, gate_failures, whisper_f32
from test_f64_statistics import check64, failures64, log_allowance, report64, stats64
from test_whisper_centered import F32_TOL, F64_TOL, make, run_split

N_FFT, HOP, PAD, SR = R.N_FFT, R.HOP, R.PAD, 16000.0
LOG10_2 = float(np.log10(2.0))
RAW_F64_GATE = 4.0 * F64_TOL        # tests/test_whisper_centered.py's gates on raw rows: the raw scale is four times the normalised one
RAW_F32_GATE = 4.0 * F32_TOL
SIXTEEN = np.float32(16.0)
PAD_SHORT = 1600


# ---- 1. inputs, frame classes, reference and yardsticks -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(64)
    long = [(0.1 * rng.standard_normal(16037)).astype(np.float32) for _ in range(40)]
    short = [(0.1 * rng.standard_normal(1000 + (37 * i) % 160)).astype(np.float32) for i in range(600)]
    for c in long + short:
        c.setflags(write=False)
    return {"long": long, "short": short}


frame_classes = R.frame_classes


def pieces(a, n, pad_to, which):
    """the frames of one clip's [T][mels] that a statistic takes, as the arrays whose row index is the slot: the interior (slot (t - 2)
    mod 6) and / or the edge frames in frame order (slot: the position among them)"""
    T, interior, first_silent = frame_classes(n, pad_to)
    assert a.shape[0] == T, (a.shape, T)
    inner, edges = a[2:2 + interior], np.concatenate([a[:min(2, first_silent)], a[2 + interior:first_silent]])
    return {"all": [inner, edges], "interior": [inner], "edges": [edges]}[which]


def cut(per_clip, lens, pad_to, which):
    return [p for a, n in zip(per_clip, lens) for p in pieces(np.asarray(a), n, pad_to, which)]


def energies(x, n_mels, pad_to=0, dtype=np.float64, window=None, bank=None):
    """the mel energies of the centred frames in numpy: reflect pad, Hann, rfft, |.|^2, bank (whisper_f32's recipe on the padded signal;
    its last frame is the one the features drop)"""
    s = R.signal(x, pad_to)
    T = R.num_frames(s.shape[0], 0)
    if T == 0:
        return np.zeros((0, n_mels), dtype)
    e = whisper_f32(np.pad(s, PAD, mode="reflect"), N_FFT, HOP, n_mels, SR, window=window, bank=bank, dtype=dtype, energies=True)[1]
    assert e.shape[0] == T + 1 and e.dtype == dtype
    return e[:T]


def ending(E, minus=SIXTEEN):
    """the kernels' declared ending on energies of either type: float32, float32 log10, + 16 rounded to float32, max(., 6), - 16"""
    with np.errstate(divide="ignore"):
        v = np.log10(np.asarray(E).astype(np.float32))
    y = np.maximum(v + SIXTEEN, np.float32(6.0)) - np.float32(minus)
    assert y.dtype == np.float32
    return y


def unbiased(E):
    y = np.log10(np.maximum(np.asarray(E).astype(np.float32), np.float32(1e-10)))
    assert y.dtype == np.float32
    return y


@functools.lru_cache(maxsize=None)
def _ref(batch, n_mels, pad_to=0):
    """-> (clips, lengths, the reference's raw rows, the f64 energies, the allowance per value), computed once and left unchanged"""
    clips = _inputs()[batch]
    lens = [c.shape[0] for c in clips]
    want = R.raw_rows_many(clips, pad_to, n_mels)
    E = [energies(c, n_mels, pad_to) for c in clips]
    L = [log_allowance(np.maximum(e, 1e-10), LOG10_2) for e in E]
    for a in want + E + L:
        a.setflags(write=False)
    return clips, lens, want, E, L


@functools.lru_cache(maxsize=None)
def _e32(batch, n_mels):
    return [energies(c, n_mels, 0, np.float32) for c in _inputs()[batch]]


def stats(batch, n_mels, which, got, yard=None, pad_to=0):
    """the statistics of per-clip rows `got` over the frames `which` against the reference, the yardstick (None: the F64 one) beside them"""
    clips, lens, want, E, L = _ref(batch, n_mels, pad_to)
    yard = [ending(e) for e in E] if yard is None else yard
    c = lambda per_clip: cut(per_clip, lens, pad_to, which)
    return stats64(c(got), c(want), c(yard), 5 if which == "edges" else 6, c(L))


# ---- 2. CPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("batch,pad_to", [("long", 0), ("short", 0), ("short", PAD_SHORT)])
def test_inputs_and_restated_energies(oracle, batch, pad_to, n_mels):
    """the numpy restatement of the f64 energies agrees with the reference to 1e-10; the clips have the frames the rows claim"""
    clips, lens, want, E, L = _ref(batch, n_mels, pad_to)
    d = max(float(np.abs(np.log10(np.maximum(e, 1e-10)) - w).max()) for e, w in zip(E, want))
    print(f"\nF64-STATS cpu-restated-{batch}-pad{pad_to}-{n_mels} max={d:.2e}")
    assert d <= 1e-10
    cls = [frame_classes(n, pad_to) for n in lens]
    assert [c[0] for c in cls] == [w.shape[0] for w in want] == [R.num_frames(n, pad_to) for n in lens]
    n_edges = [fs - it for T, it, fs in cls]
    assert MARGIN == 4.0
    if batch == "long":
        assert set(cls) == {(100, 97, 100)}
        if n_mels == 80:
            assert max(float(w.max() - w.min()) for w in want) < 8.0, "a clip spreads over 8 decades: the normalised call would clamp"
    elif pad_to == 0:
        assert set(cls) == {(6, 4, 6), (7, 4, 7)} and set(n_edges) == {2, 3} and sum(n_edges) == 1347
    else:
        assert {c[0] for c in cls} == {10} and set(n_edges) == {4, 5} and {c[2] for c in cls} == {8, 9}
        for w, e, (T, it, fs) in zip(want, E, cls):        # a silent frame is silent in the reference too
            assert np.all(w[fs:] == -10.0) and np.all(e[fs:] == 0.0)


YARDS = [("long", 0, 80, "all", "f64"), ("long", 0, 128, "all", "f64"), ("long", 0, 80, "interior", "f64"), ("long", 0, 128, "interior", "f64"),
         ("short", 0, 80, "edges", "f64"), ("short", 0, 128, "edges", "f64"), ("short", PAD_SHORT, 80, "edges", "f64"), ("short", PAD_SHORT, 128, "edges", "f64"),
         ("long", 0, 80, "all", "f32-unbiased"), ("long", 0, 80, "interior", "f32")]


@pytest.mark.parametrize("batch,pad_to,n_mels,which,kind", YARDS, ids=[f"{y[0]}-pad{y[1]}-{y[2]}-{y[3]}-{y[4]}" for y in YARDS])
def test_yardsticks_meet_the_sample_size_condition(oracle, batch, pad_to, n_mels, which, kind):
    """every yardstick a GPU row uses has a standard error of a quarter of its band bias or less (gate_failures' condition: the bias gate
    measures bias, not sample size) and passes its own gates; the un-biased F32 one beside them, as a check of the input"""
    if kind == "f64":
        yard, tol = [ending(e) for e in _ref(batch, n_mels, pad_to)[3]], RAW_F64_GATE
    else:
        yard, tol = [(ending if kind == "f32" else unbiased)(e) for e in _e32(batch, n_mels)], RAW_F32_GATE
    s = stats(batch, n_mels, which, yard, yard, pad_to)
    report64(f"cpu-yardstick-{batch}-pad{pad_to}-{n_mels}-{which}-{kind} (se / band {s[2].se / s[2].band:.2f})", s)
    assert s[2].se <= 0.25 * s[2].band, (s[2].se, s[2].band)
    assert not gate_failures(s[2], s[2], tol) and not failures64(s, tol)


def test_f32_yardstick_on_short_clips_is_sample_limited(oracle):
    """why there is no F32 row on `short`: frames that mirror at the end of the samples give the f32 evaluation a heavy tail -- printed,
    not gated; edge frames run in f64 in every mode"""
    yard = [ending(e) for e in _e32("short", 80)]
    for which in ("edges", "interior"):
        s = stats("short", 80, which, yard, yard)
        report64(f"cpu-yardstick-short-pad0-80-{which}-f32 (se / band {s[2].se / s[2].band:.2f})", s)


WRONG = ["band 41 x (1 + 1e-5)", "16 -> the next float32 above it", "edge frames: Hann tap 57 x (1 + 1e-3)"]


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("kind", WRONG)
def test_gates_are_red_on_a_subtly_wrong_evaluation(oracle, kind, n_mels):
    """the yardstick's arithmetic with one thing wrong, given the full allowance for a hardware log it does not take: red on the band
    bias; the first two stay under the 8e-6 gate that was all the raw rows had (asserted), the tap does not (module docstring)"""
    from oracle import oracle as O
    batch, which = ("short", "edges") if kind == WRONG[2] else ("long", "all")
    clips, lens, want, E, L = _ref(batch, n_mels)
    if kind == WRONG[0]:
        bad = []
        for e in E:
            e = e.copy()
            e[:, 41] *= 1.0 + 1e-5
            bad.append(ending(e))
    elif kind == WRONG[1]:
        above = np.nextafter(SIXTEEN, np.float32(17.0))
        assert 1.8e-6 < float(above) - 16.0 < 2.0e-6
        bad = [ending(e, above) for e in E]
    else:
        win = O.hann_window(N_FFT)
        win[57] *= 1.0 + 1e-3
        bad = [ending(energies(c, n_mels, window=win)) for c in clips]
    s = stats(batch, n_mels, which, bad)
    report64(f"cpu-perturbed-{n_mels}[{kind}]", s)
    missed = failures64(s, RAW_F64_GATE)
    assert "band bias" in missed and "sample size" not in missed, (kind, missed)
    if kind != WRONG[2]:
        assert "max" not in missed and s[0].max < RAW_F64_GATE, (kind, s[0].max)
    else:
        print(f"F64-STATS cpu-perturbed-{n_mels}[{kind}] max={s[0].max:.2e}: above the old gate of {RAW_F64_GATE:.0e}")
    if kind == WRONG[1]:
        assert {"mean", "slot bias"} <= set(missed), missed
    assert not failures64(stats(batch, n_mels, which, [ending(e) for e in E]), RAW_F64_GATE)


# ---- 3. GPU rows ----------------------------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def device_rows(mode, n_mels, batch, pad_to=0):
    """one split call -> (rows per clip, maxima); the maxima are the float32 maxima of the returned rows, bit for bit"""
    import mel_spec_amd as M
    clips = _inputs()[batch]
    mel = make(n_mels, mode)
    name = M.whisper_kernel_name(mel)
    assert ("six_runs_raw" in name) == (mode == "f32" and n_mels == 80), name
    assert ("six64_raw_kernel<15" in name) == (n_mels == 128), name
    rows, g = run_split(mel, clips, pad_to)
    mel.close()
    assert g.shape == (len(clips),)
    for i, r in enumerate(rows):
        assert r.shape[0] > 0
        assert same_bits(g[i], np.float32(r.max())), f"clip {i}: maximum {g[i]!r}, the largest returned value {r.max()!r}"
    return rows, g


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("mode", [None, "f64"], ids=["default", "f64"])
def test_f64_long(oracle, mode, n_mels):
    """every frame of `long` (None: the mode the suite runs in -- AUTO or F64, the f64 kernel either way), and its interior alone"""
    rows, g = device_rows(mode, n_mels, "long")
    check64(f"wc-f64-long-{mode or 'default'}-{n_mels}", stats("long", n_mels, "all", rows), RAW_F64_GATE)
    if mode == "f64":
        check64(f"wc-f64-interior-{n_mels}", stats("long", n_mels, "interior", rows), RAW_F64_GATE)


@pytest.mark.gpu
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("pad_to", [0, PAD_SHORT])
def test_edges(oracle, pad_to, n_mels):
    """the edge frames of `short`: the f64 kernel on gathered frames, the slot_map, WcEdge::row_off -- in "f64" and in "f32" mode, which must
    give the same bits on those frames (edge frames run in f64 whatever the mode)"""
    lens = [c.shape[0] for c in _inputs()["short"]]
    per_mode = {}
    for mode in ("f64", "f32"):
        rows, g = device_rows(mode, n_mels, "short", pad_to)
        check64(f"wc-edges-{mode}-pad{pad_to}-{n_mels}", stats("short", n_mels, "edges", rows, pad_to=pad_to), RAW_F64_GATE)
        per_mode[mode] = cut(rows, lens, pad_to, "edges")
        for r, n in zip(rows, lens):
            assert np.all(r[frame_classes(n, pad_to)[2]:] == np.float32(-10.0)), "a silent frame is not exactly -10"
    for a, b in zip(per_mode["f64"], per_mode["f32"]):
        assert same_bits(a, b), "an edge frame differs between the modes"


@pytest.mark.gpu
def test_f32_interior(oracle):
    """the f32 run kernel's raw rows on the interior of `long` against the F32 yardstick"""
    rows, g = device_rows("f32", 80, "long")
    yard = [ending(e) for e in _e32("long", 80)]
    check64("wc-f32-interior-80", stats("long", 80, "interior", rows, yard), RAW_F32_GATE)
