"""The centred Whisper features (melspec_whisper_*: reflect-padded STFT, pad / trim to pad_to, clamp against the maximum of the whole clip)
on the GPU against tests/whisper_centered_ref.py, compared whole: every value of every clip, outputs fenced with guard words.

Gates, taken from tests/test_whole_batch.py: F64_TOL = 2e-6 on normalised values in AUTO and F64 (both run the f64 kernel here), F32_TOL =
6e-4 in F32 -- a clip-wide clamp is never below the per-frame clamp, so for every band the new error is at most the old one plus the error
of g.  Raw rows of the split calls are compared directly in F64 only, at 4 x F64_TOL (the raw scale is four times the normalised one); in
F32 after folding step 6 in numpy.  The fold of the split output against the normalised call: 5e-7, two f32 ulps at magnitude 2.

Every check_batch also asserts that a clip's returned maximum is, bit for bit, the float32 maximum of its returned raw rows (both are
`biased - 16.0f` of the same bits).  run_norm / run_split take caller-chosen output offsets and a shift of the output pointer, and check
that every float outside the clips' outputs keeps its sentinel.  The statistics of the raw rows: tests/test_whisper_centered_stats.py."""
import ctypes as C

import numpy as np
import pytest
import torch   # before libmelspec_hip.so is loaded (tests/test_full_size.py); a caller's stream comes from here

import mel_spec_amd as M
import whisper_centered_ref as R

F64_TOL = 2e-6
F32_TOL = 6e-4
FOLD_TOL = 5e-7
GUARD = 64                  # guard floats either side of every device output (256 bytes: the fenced buffer keeps its 16-byte alignment)
SENTINEL = np.float32(-777.25)

PLAIN = [400, 401, 559, 560, 599, 600, 639, 640, 679, 680, 1119, 1120, 1360, 1520]
PADDED = [0, 1, 199, 200, 201, 399, 400, 2400, 4599, 4600, 4601, 4799, 4800, 9000]

pytestmark = pytest.mark.gpu


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------------
class Fenced:
    """a device output of n floats between two runs of guard words"""

    def __init__(self, n):
        from mel_spec_amd.hip import DeviceBuffer
        self.n = int(n)
        self.buf = DeviceBuffer((self.n + 2 * GUARD) * 4)
        self.buf.upload(np.full(self.n + 2 * GUARD, SENTINEL, np.float32))
        self.ptr = self.buf.ptr + GUARD * 4

    def get(self):
        a = self.buf.download((self.n + 2 * GUARD,))
        assert np.all(a[:GUARD] == SENTINEL) and np.all(a[GUARD + self.n:] == SENTINEL), "guard words overwritten"
        return a[GUARD:GUARD + self.n]

    def free(self):
        self.buf.free()


def make(n_mels=80, mode=None):
    mel = M.HipMelSpectrogram(400, 160, 16000.0, n_mels, device=0)
    if mode:
        mel.set_precision(mode)
    return mel


def upload(clips):
    from mel_spec_amd.hip import DeviceBuffer, _flatten
    flat, offs, lens = _flatten(clips)
    d = DeviceBuffer(flat.nbytes)
    d.upload(flat)
    return d, offs, lens


def _place(Ts, n_mels, offsets):
    """where each clip's T_i x n_mels floats start (None: packed in clip order) and the floats the whole output spans"""
    sizes = [T * n_mels for T in Ts]
    if offsets is None:
        offsets = [int(v) for v in np.concatenate([[0], np.cumsum(sizes)[:-1]])] if sizes else []
    offsets = [int(o) for o in offsets]
    return offsets, sizes, max([o + n for o, n in zip(offsets, sizes)] + [0])


def _collect(flat, offsets, sizes, shift):
    """the clips' floats out of a downloaded output; every float the call had no business with -- the `shift` floats in front of the
    pointer it was given and the gaps between caller-chosen offsets -- still holds the sentinel"""
    used = np.zeros(flat.shape[0], bool)
    for o, n in zip(offsets, sizes):
        assert not used[shift + o:shift + o + n].any(), "the test's own offsets overlap"
        used[shift + o:shift + o + n] = True
    assert np.all(flat[~used] == SENTINEL), "a float outside the clips' outputs was overwritten"
    return [flat[shift + o:shift + o + n] for o, n in zip(offsets, sizes)]


def run_norm(mel, clips, pad_to, mel_major, stream=0, out_offsets=None, shift=0):
    """the ragged normalised call -> list of [T_i][n_mels] (mel-major results transposed back).  out_offsets: h_out_offsets, in floats;
    shift: d_out is advanced by that many floats past the fenced buffer's 16-byte aligned start"""
    d, offs, lens = upload(clips)
    Ts = [R.num_frames(int(n), pad_to) for n in lens]
    where, sizes, span = _place(Ts, mel.n_mels, out_offsets)
    out = Fenced(span + shift)
    try:
        M.whisper_ragged_device(mel, d.ptr, offs, lens, out.ptr + 4 * shift, pad_to, None if out_offsets is None else where, mel_major, stream)
        mel.synchronize(stream)
        parts = _collect(out.get(), where, sizes, shift)
    finally:
        d.free(); out.free()
    return [a.reshape(mel.n_mels, T).T.copy() if mel_major else a.reshape(T, mel.n_mels).copy() for a, T in zip(parts, Ts)]


def run_split(mel, clips, pad_to, d_max=None, rows_offsets=None, shift=0):
    """the ragged split call -> (list of raw rows [T_i][n_mels], g [n_clips]); d_max: a Fenced to use (and keep) for the maxima;
    rows_offsets: h_rows_offsets, in floats; shift: as in run_norm, for d_rows"""
    d, offs, lens = upload(clips)
    Ts = [R.num_frames(int(n), pad_to) for n in lens]
    where, sizes, span = _place(Ts, mel.n_mels, rows_offsets)
    rows = Fenced(span + shift)
    mx = d_max or Fenced(len(clips))
    try:
        M.whisper_ragged_device_split(mel, d.ptr, offs, lens, rows.ptr + 4 * shift, mx.ptr, pad_to, None if rows_offsets is None else where)
        mel.synchronize()
        parts, g = _collect(rows.get(), where, sizes, shift), mx.get().copy()
    finally:
        d.free(); rows.free()
        if d_max is None:
            mx.free()
    return [a.reshape(T, mel.n_mels).copy() for a, T in zip(parts, Ts)], g


_REF = {}


def ref(key, clips, pad_to, n_mels):
    """the reference of a batch, computed once per session and left unchanged: list of (raw, g, normalised)"""
    k = (key, pad_to, n_mels)
    if k not in _REF:
        raws = R.raw_rows_many(clips, pad_to, n_mels)
        out = []
        for raw in raws:
            g, nrm = R.normalise(raw)
            raw.setflags(write=False); nrm.setflags(write=False)
            out.append((raw, g, nrm))
        _REF[k] = out
    return _REF[k]


def worst(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got.astype(np.float64) - want).max()) if want.size else 0.0


def check_batch(mel, key, clips, pad_to, tol, raw_direct, what):
    """normalised (both layouts), split, split folded against normalised -- every clip whole"""
    want = ref(key, clips, pad_to, mel.n_mels)
    mm = run_norm(mel, clips, pad_to, True)
    fm = run_norm(mel, clips, pad_to, False)
    rows, g = run_split(mel, clips, pad_to)
    w_n = w_r = w_g = w_f = 0.0
    for i, (raw, gw, nrm) in enumerate(want):
        assert np.array_equal(mm[i], fm[i]), f"{what}: clip {i}: mel-major and frame-major bits differ"
        w_n = max(w_n, worst(fm[i], nrm))
        w_g = max(w_g, abs(float(g[i]) - gw))
        if raw.shape[0]:          # the maximum is `biased - 16.0f` of the bits of one of the stored values: exactly the largest of them
            assert g[i] == np.float32(rows[i].max()), f"{what}: clip {i}: maximum {g[i]!r}, the largest returned value {rows[i].max()!r}"
        folded = R.fold_f32(rows[i], g[i])
        w_f = max(w_f, worst(folded, fm[i].astype(np.float64)))
        if raw_direct:
            w_r = max(w_r, worst(rows[i], raw))
        else:
            w_r = max(w_r, worst(folded, nrm))
    print(f"{what}: normalised {w_n:.3e} (gate {tol:.0e}), g {w_g:.3e}, split {'raw' if raw_direct else 'folded'} {w_r:.3e}, fold vs normalised {w_f:.3e}")
    assert w_n <= tol, f"{what}: normalised"
    assert w_g <= 4 * tol, f"{what}: clip maxima"
    assert w_r <= (4 * tol if raw_direct else tol), f"{what}: split rows"
    assert w_f <= FOLD_TOL, f"{what}: split folded against the normalised call"
    return fm, rows, g


def noise(clip, n, oracle):
    return oracle.synth_pcm(clip, n) if n else np.zeros(0, np.float32)


# ---- frame counts through the library ---------------------------------------------------------------------------------------------------
def test_num_frames(oracle):
    for nm in (80, 128):
        mel = make(nm)
        assert M.supports_whisper(mel)
        for n in [399] + PLAIN:
            assert M.whisper_num_frames(mel, n, 0) == R.num_frames(n, 0), n
        for n in PADDED + [4801]:
            assert M.whisper_num_frames(mel, n, 4800) == R.num_frames(n, 4800) == 30, n
        assert M.whisper_num_frames(mel, 176000) == 3000 and M.whisper_num_frames(mel, 176000, 0) == 1100
        assert M.whisper_num_frames(mel, 1000, 399) == 0
        mel.close()


# ---- clip lengths: reflection left, and right on / off at n % 160 = 39 / 40; interiors of 0, 1, 2, 6 and 7 frames ------------------------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_clip_lengths(oracle, n_mels):
    clips = [noise(100 + i, n, oracle) for i, n in enumerate(PLAIN)]
    for mode, tol in ((None, F64_TOL), ("f32", F32_TOL)):          # None: the mode the suite runs in (AUTO or F64: the f64 kernel)
        mel = make(n_mels, mode)
        for i, c in enumerate(clips):          # one clip each
            check_batch(mel, ("len", PLAIN[i]), [c], 0, tol, mode != "f32", f"n {PLAIN[i]} mels {n_mels} mode {mode}")
        mel.close()


# ---- padding and trimming: all-silent, straddling frames, reflection of real samples at the right end only past pad_to - 200, trim --------
@pytest.mark.parametrize("n_mels", [80, 128])
def test_pad_and_trim(oracle, n_mels):
    clips = [noise(200 + i, n, oracle) for i, n in enumerate(PADDED)]
    for mode, tol in ((None, F64_TOL), ("f32", F32_TOL)):          # None: the mode the suite runs in (AUTO or F64: the f64 kernel)
        mel = make(n_mels, mode)
        for i, c in enumerate(clips):
            fm, rows, g = check_batch(mel, ("pad", PADDED[i]), [c], 4800, tol, mode != "f32", f"pad_to 4800 n {PADDED[i]} mels {n_mels} mode {mode}")
            assert fm[0].shape == (30, n_mels)
            if PADDED[i] == 0:
                assert np.all(fm[0] == np.float32(-1.5)) and np.all(rows[0] == np.float32(-10.0)) and g[0] == np.float32(-10.0)
        # the whole set as one batch: every clip the same T
        check_batch(mel, "pad-all", clips, 4800, tol, mode != "f32", f"pad_to 4800, all lengths in one batch, mels {n_mels} mode {mode}")
        mel.close()


@pytest.mark.parametrize("n_mels", [80, 128])
def test_jfk_30s(jfk, n_mels):
    mel = make(n_mels)
    want = ref("jfk", [jfk], 480000, n_mels)[0][2]
    got = M.whisper_features(mel, jfk)                      # the host call, mel-major, pad_to = 480000
    assert got.shape == (n_mels, 3000)
    d = worst(got.T, want)
    print(f"JFK 30 s, {n_mels} mels: {d:.3e}")
    assert d <= F64_TOL
    assert np.array_equal(got, run_norm(mel, [jfk], 480000, True)[0].T)
    fm = M.whisper_features(mel, jfk, 0, False)
    assert fm.shape == (1100, n_mels) and worst(fm, ref("jfk", [jfk], 0, n_mels)[0][2]) <= F64_TOL
    if n_mels == 80:
        mel.set_precision("f32")
        d32 = worst(M.whisper_features(mel, jfk).T, want)
        print(f"JFK 30 s, F32: {d32:.3e}")
        assert d32 <= F32_TOL
    mel.close()


# ---- where the maximum sits: a full-scale burst in noise at 1e-3, 30 s so that the maximum crosses workgroups -------------------------------
def _burst_clip(oracle, centre, n=480000):
    x = (oracle.synth_pcm(7, n) * np.float32(1e-3)).astype(np.float32)
    lo = max(0, centre - 200)
    hi = min(n, centre + 200)
    x[lo:hi] = oracle.synth_pcm(8, hi - lo)
    return x


@pytest.mark.parametrize("where", ["frame0", "frame1", "last", "first_unit", "last_unit"])
def test_where_the_maximum_sits(oracle, where):
    T = 3000
    t = {"frame0": 0, "frame1": 1, "last": T - 1, "first_unit": 4, "last_unit": T - 4}[where]
    x = _burst_clip(oracle, 160 * t)
    mel = make(80)
    fm, rows, g = check_batch(mel, ("burst", where), [x], 0, F64_TOL, True, f"burst at frame {t}")
    raw = ref(("burst", where), [x], 0, 80)[0][0]
    assert abs(int(np.argmax(raw.max(axis=1))) - t) <= 1, "the reference's maximum is not where the burst is"
    assert int(np.argmax(rows[0].max(axis=1))) == int(np.argmax(raw.max(axis=1)))
    mel.set_precision("f32")
    check_batch(mel, ("burst", where), [x], 0, F32_TOL, False, f"burst at frame {t}, F32")
    mel.close()


def test_burst_in_the_trimmed_samples(oracle):
    """the maximum must not see samples that pad_to trims away"""
    x = (oracle.synth_pcm(7, 9000) * np.float32(1e-3)).astype(np.float32)
    x[6000:6400] = oracle.synth_pcm(8, 400)
    mel = make(80)
    fm, rows, g = check_batch(mel, "trimmed-burst", [x], 4800, F64_TOL, True, "burst past pad_to")
    quiet = ref("trimmed-burst-quiet", [x[:4800]], 4800, 80)[0]
    assert abs(float(g[0]) - quiet[1]) <= 4 * F64_TOL and worst(fm[0], quiet[2]) <= F64_TOL
    mel.close()


# ---- runs across clips: more than two clips per workgroup, runs that enter a new clip mid-wave ------------------------------------------------
def _ragged_1100(oracle):
    rng = np.random.RandomState(20261021)
    units = rng.randint(1, 10, size=1100)
    extra = rng.randint(0, 160, size=1100)
    clips = []
    for i in range(1100):
        n = 520 + 160 * (6 * int(units[i]) - 1) + int(extra[i])          # an interior of exactly units[i] six-frame units, any tail
        clips.append((oracle.synth_pcm(1000 + i, n) * np.float32(2.0 ** -(i & 7))).astype(np.float32))
    return clips


@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_ragged_1100(oracle, mode):
    clips = _ragged_1100(oracle)
    mel = make(80, mode)
    tol = F64_TOL if mode == "f64" else F32_TOL
    fm, rows, g = check_batch(mel, "ragged-1100", clips, 0, tol, mode == "f64", f"1100 ragged clips, {mode}")
    want = ref("ragged-1100", clips, 0, 80)
    gw = np.array([w[1] for w in want])
    assert np.abs(g - gw).max() <= 4 * tol
    assert len(set(np.round(gw[:8], 3))) == 8, "neighbouring clips have different maxima"
    mel.close()


# ---- stale state, repeatability ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f64", "f32"])
def test_stale_state_and_same_bits(oracle, mode):
    lens = [1360, 5000, 1520, 9000, 700, 400]
    loud = [noise(300 + i, n, oracle) for i, n in enumerate(lens)]
    quiet = [(c * np.float32(1e-3)).astype(np.float32) for c in loud]          # 60 dB down
    mel = make(80, mode)
    mx = Fenced(len(lens))
    run_norm(mel, loud, 0, True)
    run_split(mel, loud, 0, mx)
    rows_q, g_q = run_split(mel, quiet, 0, mx)           # the same d_clip_max and context, now for the quiet batch
    norm_q = run_norm(mel, quiet, 0, True)
    mx.free()
    fresh = make(80, mode)
    rows_f, g_f = run_split(fresh, quiet, 0)
    norm_f = run_norm(fresh, quiet, 0, True)
    assert np.array_equal(g_q, g_f)
    for a, b in zip(rows_q + norm_q, rows_f + norm_f):
        assert np.array_equal(a, b), "a used context differs from a fresh one"
    # the same batch twice: the same bits
    again = run_norm(mel, quiet, 0, True)
    for a, b in zip(norm_q, again):
        assert np.array_equal(a, b)
    # a clip alone and inside a batch: the same bits
    for i in (0, 3, 5):
        alone = run_norm(fresh, [quiet[i]], 0, True)[0]
        assert np.array_equal(alone, norm_q[i]), f"clip {i} alone differs from the clip inside the batch"
        r1, g1 = run_split(fresh, [quiet[i]], 0)
        assert np.array_equal(r1[0], rows_q[i]) and g1[0] == g_q[i]
    mel.close(); fresh.close()


def test_uniform_calls_and_streams(oracle):
    """the uniform calls against the ragged ones; the context's stream and a caller's"""
    from mel_spec_amd.hip import DeviceBuffer
    n, k = 2400, 5
    clips = [noise(400 + i, n, oracle) for i in range(k)]
    mel = make(80)
    want = run_norm(mel, clips, 4800, True)
    rows_w, g_w = run_split(mel, clips, 4800)
    d = DeviceBuffer(n * k * 4)
    d.upload(np.concatenate(clips))
    side = torch.cuda.Stream()
    for stream in (0, side.cuda_stream):
        out, rows, mx = Fenced(k * 30 * 80), Fenced(k * 30 * 80), Fenced(k)
        M.whisper_uniform_device(mel, d.ptr, n, n, k, out.ptr, 4800, True, stream)
        M.whisper_uniform_device_split(mel, d.ptr, n, n, k, rows.ptr, mx.ptr, 4800, stream)
        mel.synchronize(stream)
        o, r, g = out.get().reshape(k, 80, 30), rows.get().reshape(k, 30, 80), mx.get()
        for i in range(k):
            assert np.array_equal(o[i].T, want[i]) and np.array_equal(r[i], rows_w[i])
        assert np.array_equal(g, g_w)
        out.free(); rows.free(); mx.free()
    # the batch helpers of the Python frontend
    feats = M.whisper_features_batch(mel, clips, 4800)
    rows_b, g_b = M.whisper_split(mel, clips, 4800)
    for i in range(k):
        assert np.array_equal(feats[i].T, want[i]) and np.array_equal(rows_b[i], rows_w[i])
    assert np.array_equal(g_b, g_w)
    mel.release_scratch()
    assert np.array_equal(M.whisper_features_batch(mel, clips, 4800)[0].T, want[0])
    d.free(); mel.close()


# ---- arguments -------------------------------------------------------------------------------------------------------------------------------
def test_arguments(oracle):
    from mel_spec_amd import _lib
    from mel_spec_amd.hip import HipRuntimeError
    x = noise(1, 4800, oracle)
    for args in ((512, 160, 80), (400, 160, 40), (400, 200, 80)):
        other = M.HipMelSpectrogram(args[0], args[1], 16000.0, args[2], device=0)
        assert not M.supports_whisper(other) and M.whisper_num_frames(other, 4800, 0) == 0 and M.whisper_kernel_name(other) == ""
        d, offs, lens = upload([x])
        out = Fenced(30 * args[2])
        with pytest.raises(HipRuntimeError) as e:
            M.whisper_ragged_device(other, d.ptr, offs, lens, out.ptr, 0)
        assert e.value.code == _lib.ERR_UNSUPPORTED
        assert np.all(out.get() == SENTINEL), "an unsupported context touched its output"
        host = np.full(30 * args[2], SENTINEL, np.float32)
        nf = C.c_size_t(7)
        rc = _lib.lib().melspec_whisper_compute_host(other._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, 0, host.ctypes.data_as(C.POINTER(C.c_float)),
                                                     host.size, 1, C.byref(nf))
        assert rc == _lib.ERR_UNSUPPORTED and nf.value == 0 and np.all(host == SENTINEL)
        d.free(); out.free(); other.close()
    mel = make(80)
    d, offs, lens = upload([x])
    out, mx = Fenced(30 * 80), Fenced(1)
    for pad in (1, 399):
        with pytest.raises(HipRuntimeError) as e:
            M.whisper_ragged_device(mel, d.ptr, offs, lens, out.ptr, pad)
        assert e.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(HipRuntimeError) as e:
            M.whisper_uniform_device_split(mel, d.ptr, 4800, 4800, 1, out.ptr, mx.ptr, pad)
        assert e.value.code == _lib.ERR_INVALID_ARG
        with pytest.raises(HipRuntimeError):
            M.whisper_features(mel, x, pad)
    with pytest.raises(HipRuntimeError) as e:
        M.whisper_uniform_device_split(mel, d.ptr, 4800, 4800, 1, out.ptr, 0, 0)
    assert e.value.code == _lib.ERR_INVALID_ARG
    with pytest.raises(HipRuntimeError) as e:
        M.whisper_uniform_device(mel, 0, 4800, 4800, 1, out.ptr, 0)
    assert e.value.code == _lib.ERR_INVALID_ARG
    assert np.all(out.get() == SENTINEL) and np.all(mx.get() == SENTINEL)
    # a clip without frames: nothing is written but its maximum
    M.whisper_uniform_device_split(mel, d.ptr, 399, 399, 1, out.ptr, mx.ptr, 0)
    mel.synchronize()
    assert np.all(out.get() == SENTINEL) and mx.get()[0] == np.float32(-10.0)
    # capacity on the host call
    host = np.full(30 * 80, SENTINEL, np.float32)
    nf = C.c_size_t(7)
    rc = _lib.lib().melspec_whisper_compute_host(mel._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, 0, host.ctypes.data_as(C.POINTER(C.c_float)),
                                                 30 * 80 - 1, 1, C.byref(nf))
    assert rc == _lib.ERR_CAPACITY and nf.value == 0 and np.all(host == SENTINEL)
    rc = _lib.lib().melspec_whisper_compute_host(mel._h, x.ctypes.data_as(C.POINTER(C.c_float)), x.size, 0, host.ctypes.data_as(C.POINTER(C.c_float)),
                                                 30 * 80, 1, C.byref(nf))
    assert rc == 0 and nf.value == 30 and worst(host.reshape(80, 30).T, ref("args", [x], 0, 80)[0][2]) <= F64_TOL
    assert "six64_raw" in M.whisper_kernel_name(mel)
    mel.set_precision("f32")
    assert "six_runs_raw" in M.whisper_kernel_name(mel)
    d.free(); out.free(); mx.free(); mel.close()


# ---- the finalise pass's tiles of 64 frames: full and partial last tiles, the 16-byte path on and off, the live / silent boundary in and on a tile ----
MODES = [(80, None, F64_TOL), (80, "f32", F32_TOL), (128, None, F64_TOL)]          # None: the mode the suite runs in (the f64 kernel)
MODE_IDS = ["80-f64", "80-f32", "128-f64"]
TILE_T = [63, 64, 65, 66, 67, 68, 127, 128, 129, 132]
TILE_PADS = {10240: 64, 10880: 68, 20480: 128}
TILE_PAD_N = [0, 1000, 10040, 10239, 20000]


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def _shifted(mel, clips, pad_to, fm, rows, g, what):
    """the same calls with the output pointer one and two floats past its 16-byte aligned start: the same bits, nothing outside them"""
    for shift in (1, 2):
        for mel_major in (True, False):
            got = run_norm(mel, clips, pad_to, mel_major, shift=shift)
            assert all(same(a, b) for a, b in zip(got, fm)), f"{what}: d_out + {shift} floats, mel_major {mel_major}"
        r, gg = run_split(mel, clips, pad_to, shift=shift)
        assert all(same(a, b) for a, b in zip(r, rows)) and np.array_equal(gg, g), f"{what}: d_rows + {shift} floats"


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_finalize_tiles(oracle, n_mels, mode, tol):
    """T around one and two tiles, at pad_to = 0 (n = 160 T): each clip alone, then all of them as one batch"""
    clips = [noise(500 + T, 160 * T, oracle) for T in TILE_T]
    mel = make(n_mels, mode)
    alone = []
    for T, c in zip(TILE_T, clips):
        assert R.frame_classes(c.shape[0], 0) == (T, T - 3, T)
        fm, rows, g = check_batch(mel, ("tile", T), [c], 0, tol, mode != "f32", f"T {T} mels {n_mels} mode {mode}")
        assert fm[0].shape == (T, n_mels)
        alone.append((fm[0], rows[0], g[0]))
        if T in (64, 68, 128):
            _shifted(mel, [c], 0, fm, rows, g, f"T {T}")
    fm, rows, g = check_batch(mel, "tile-all", clips, 0, tol, mode != "f32", f"T {TILE_T} in one batch, mels {n_mels} mode {mode}")
    for i, (a, r, m) in enumerate(alone):
        assert same(fm[i], a) and same(rows[i], r) and g[i] == m, f"T {TILE_T[i]} alone differs from the clip inside the batch"
    mel.close()


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_finalize_tiles_at_the_silent_boundary(oracle, n_mels, mode, tol):
    """pad_to of exactly one tile, a tile and four frames, two tiles: every frame silent, the boundary inside the first tile, exactly on the
    tile's edge (first_silent == 64), two frames past it, and (pad_to 20480) near the end of the second tile"""
    clips = [noise(600 + i, n, oracle) for i, n in enumerate(TILE_PAD_N)]
    mel = make(n_mels, mode)
    for pad_to, T in TILE_PADS.items():
        cls = [R.frame_classes(n, pad_to) for n in TILE_PAD_N]
        assert [c[0] for c in cls] == [T] * len(clips)
        assert [c[2] for c in cls] == [0, 8, 64, min(66, T), min(127, T)], cls
        fm, rows, g = check_batch(mel, ("tile-pad", pad_to), clips, pad_to, tol, mode != "f32", f"pad_to {pad_to} n {TILE_PAD_N} mels {n_mels} mode {mode}")
        for i, c in enumerate(cls):
            assert np.all(rows[i][c[2]:] == np.float32(-10.0)), "a silent frame's raw row is not exactly -10"
            lo = np.float32(np.float32(g[i]) - np.float32(8.0))
            assert np.all(fm[i][c[2]:] == (np.maximum(np.float32(-10.0), lo) + np.float32(4.0)) * np.float32(0.25)), "a silent frame's normalised row"
        _shifted(mel, clips, pad_to, fm, rows, g, f"pad_to {pad_to}")
    mel.close()


# ---- caller-chosen output offsets: h_out_offsets / h_rows_offsets -----------------------------------------------------------------------------
def _gapped(Ts, n_mels, gaps, order):
    """offsets, in floats, that lay the clips out in `order` with gaps[k] spare floats in front of the k-th one laid down"""
    offs, cur = [0] * len(Ts), 0
    for k, i in enumerate(order):
        cur += gaps[k]
        offs[i] = cur
        cur += Ts[i] * n_mels
    return offs


@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("pad_to", [0, 10240])
def test_caller_chosen_offsets(oracle, pad_to, n_mels):
    """the packed call's bits, clip by clip, wherever the caller puts them -- in clip order and reversed, with gaps that leave some clips'
    first float off a multiple of four (the mel-major 16-byte path is off for them: T = 64, 68, 128 among them) and some on one; every
    float of every gap keeps its sentinel (run_norm / run_split check that).  pad_to 10240: T = 64 for all, with all-silent clips and
    silent tails -- the fill pass on caller-chosen offsets"""
    lens = [160 * 64, 160 * 128 + 35, 5000, 160 * 68, 1360, 160 * 100 + 7] if pad_to == 0 else [1000, 10040, 0, 5000, 20000, 10239]
    clips = [noise(800 + i, n, oracle) for i, n in enumerate(lens)]
    Ts = [R.num_frames(n, pad_to) for n in lens]
    assert Ts == ([64, 128, 31, 68, 8, 100] if pad_to == 0 else [64] * 6)
    mel = make(n_mels)
    fm, rows, g = check_batch(mel, ("offsets", pad_to), clips, pad_to, F64_TOL, True, f"offsets: the packed call, pad_to {pad_to} mels {n_mels}")
    for order in (list(range(6)), list(range(5, -1, -1))):
        offs = _gapped(Ts, n_mels, [0, 1, 3, 5, 2, 7], order)
        full = [(o & 3) for o, T in zip(offs, Ts) if T % 4 == 0 and T >= 64]
        assert 0 in full and any(full), "the offsets do not turn the 16-byte path both on and off"
        for mel_major in (True, False):
            got = run_norm(mel, clips, pad_to, mel_major, out_offsets=offs)
            for i in range(6):
                assert same(got[i], fm[i]), f"clip {i} at float {offs[i]}, mel_major {mel_major}"
        r, gg = run_split(mel, clips, pad_to, rows_offsets=offs)
        for i in range(6):
            assert same(r[i], rows[i]), f"clip {i}: raw rows at float {offs[i]}"
        assert np.array_equal(gg, g)
    mel.close()


# ---- the uniform calls: a stride past the clip, a stride of zero, trimming more than one clip ---------------------------------------------------
def _uniform(mel, d_ptr, stride, n, k, pad_to):
    """the three uniform calls -> (mel-major transposed back [k][T][mels], frame-major, raw rows, maxima)"""
    T, nm = R.num_frames(n, pad_to), mel.n_mels
    mm, fm, rows, mx = Fenced(k * T * nm), Fenced(k * T * nm), Fenced(k * T * nm), Fenced(k)
    try:
        M.whisper_uniform_device(mel, d_ptr, stride, n, k, mm.ptr, pad_to, True)
        M.whisper_uniform_device(mel, d_ptr, stride, n, k, fm.ptr, pad_to, False)
        M.whisper_uniform_device_split(mel, d_ptr, stride, n, k, rows.ptr, mx.ptr, pad_to)
        mel.synchronize()
        return mm.get().reshape(k, nm, T).transpose(0, 2, 1), fm.get().reshape(k, T, nm), rows.get().reshape(k, T, nm), mx.get().copy()
    finally:
        mm.free(); fm.free(); rows.free(); mx.free()


def test_uniform_strides_and_trim(oracle):
    from mel_spec_amd.hip import DeviceBuffer
    n, k = 2400, 5
    clips = [noise(400 + i, n, oracle) for i in range(k)]
    mel = make(80)
    # clip_stride > clip_len: what lies between the clips is not the call's to read (1e3 there would be heard in every edge frame)
    stride = n + 37
    buf = np.full(stride * k, 1e3, np.float32)
    for i, c in enumerate(clips):
        buf[i * stride:i * stride + n] = c
    d = DeviceBuffer(buf.nbytes)
    d.upload(buf)
    for pad_to in (0, 4800):
        fm_w, rows_w, g_w = check_batch(mel, "uniform-5", clips, pad_to, F64_TOL, True, f"five clips of 2400, pad_to {pad_to}")
        mm, fm, rows, g = _uniform(mel, d.ptr, stride, n, k, pad_to)
        for i in range(k):
            assert same(mm[i], fm_w[i]) and same(fm[i], fm_w[i]) and same(rows[i], rows_w[i]), f"stride {stride}, pad_to {pad_to}, clip {i}"
        assert np.array_equal(g, g_w)
        # clip_stride == 0: the same clip n_clips times
        mm, fm, rows, g = _uniform(mel, d.ptr, 0, n, 3, pad_to)
        for i in range(3):
            assert same(mm[i], fm_w[0]) and same(fm[i], fm_w[0]) and same(rows[i], rows_w[0]) and g[i] == g_w[0], f"stride 0, pad_to {pad_to}, copy {i}"
    d.free()
    # trim: clip_len > pad_to, more than one clip
    d = DeviceBuffer(n * k * 4)
    d.upload(np.concatenate(clips))
    cut = [c[:1600] for c in clips]
    fm_w, rows_w, g_w = check_batch(mel, "uniform-5-trimmed", cut, 1600, F64_TOL, True, "five clips of 2400 trimmed to 1600")
    mm, fm, rows, g = _uniform(mel, d.ptr, n, n, k, 1600)
    assert fm.shape == (k, 10, 80)
    for i in range(k):
        assert same(mm[i], fm_w[i]) and same(fm[i], fm_w[i]) and same(rows[i], rows_w[i]), f"trimmed clip {i}"
    assert np.array_equal(g, g_w)
    d.free()
    # the host call trims too
    x = noise(410, 9000, oracle)
    assert same(M.whisper_features(mel, x, 4800), M.whisper_features(mel, x[:4800], 4800))
    assert same(M.whisper_features(mel, x, 4800).T, run_norm(mel, [x[:4800]], 4800, True)[0])
    mel.close()


# ---- a clip without a frame in the middle of a batch that has frames ------------------------------------------------------------------------
@pytest.mark.parametrize("mode,tol", [(None, F64_TOL), ("f32", F32_TOL)], ids=["f64", "f32"])
def test_clips_without_a_frame_inside_a_batch(oracle, mode, tol):
    lens = [1360, 0, 399, 700, 200, 5000]
    clips = [noise(900 + i, n, oracle) for i, n in enumerate(lens)]
    mel = make(80, mode)
    fm, rows, g = check_batch(mel, "frameless", clips, 0, tol, mode != "f32", f"lengths {lens}, mode {mode}")
    for i in (1, 2, 4):
        assert g[i] == np.float32(-10.0) and rows[i].shape == (0, 80) and fm[i].shape == (0, 80)
    for i in (0, 3, 5):          # their rows and words are where they would be without the frameless clips between them
        for mel_major in (True, False):
            assert same(run_norm(mel, [clips[i]], 0, mel_major)[0], fm[i]), f"clip {i} alone, mel_major {mel_major}"
        r1, g1 = run_split(mel, [clips[i]], 0)
        assert same(r1[0], rows[i]) and g1[0] == g[i], f"clip {i} alone: raw rows / maximum"
    mel.close()


# ---- 128 mels (the 15-slot f64 kernel) with runs that cross clips; F32 mode at 128 mels is the f64 kernel ----------------------------------------
def test_ragged_1100_at_128_mels(oracle):
    clips = _ragged_1100(oracle)
    mel = make(128, "f64")
    assert "six64_raw_kernel<15" in M.whisper_kernel_name(mel)
    fm, rows, g = check_batch(mel, "ragged-1100", clips, 0, F64_TOL, True, "1100 ragged clips, 128 mels, f64")
    mel.set_precision("f32")
    assert "six64_raw_kernel<15" in M.whisper_kernel_name(mel) and "six_runs_raw" not in M.whisper_kernel_name(mel)
    fm32 = run_norm(mel, clips, 0, True)
    rows32, g32 = run_split(mel, clips, 0)
    for i in range(len(clips)):
        assert same(fm32[i], fm[i]) and same(rows32[i], rows[i]), f"clip {i}: F32 mode at 128 mels differs from F64 mode"
    assert np.array_equal(g32, g)
    mel.close()


# ---- pad_to other than 4800 / 480000 on the device --------------------------------------------------------------------------------------------
DEVICE_PADS = [400, 401, 559, 560, 4799, 4801, 4959]


def _pad_lengths(pad_to):
    ns = [0, 1, 200, 399, 400, 560, pad_to - 201, pad_to - 200, pad_to - 1, pad_to, pad_to + 1, pad_to + 500]
    return [n for k, n in enumerate(ns) if n >= 0 and n not in ns[:k]]


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_pad_to_on_the_device(oracle, n_mels, mode, tol):
    mel = make(n_mels, mode)
    for pad_to in DEVICE_PADS:
        lens = _pad_lengths(pad_to)
        for n in lens:
            assert M.whisper_num_frames(mel, n, pad_to) == R.num_frames(n, pad_to) == pad_to // 160
        clips = [noise(1200 + i, n, oracle) for i, n in enumerate(lens)]
        check_batch(mel, ("device-pad", pad_to), clips, pad_to, tol, mode != "f32", f"pad_to {pad_to} n {lens} mels {n_mels} mode {mode}")
    mel.close()


# ---- quiet input: values on the 1e-10 floor, a hole of digital silence in the interior of a loud clip --------------------------------------------
QUIET = ["1e-4", "1e-5", "1e-6", "hole"]


def _quiet_clips():
    x = np.random.default_rng(9000).standard_normal(9000)
    clips = [(s * x).astype(np.float32) for s in (1e-4, 1e-5, 1e-6)]
    hole = (0.1 * x).astype(np.float32)
    hole[3000:6000] = 0.0          # frames 20 .. 36 of 56 read zeros only; they are interior: transformed, not filled
    return clips + [hole]


@pytest.mark.parametrize("n_mels,mode,tol", MODES, ids=MODE_IDS)
def test_quiet_input(oracle, n_mels, mode, tol):
    clips = _quiet_clips()
    want = ref("quiet", clips, 0, n_mels)
    on_floor = [float(np.mean(w[0] == -10.0)) for w in want]
    print(f"quiet input, {n_mels} mels: share of the reference's values on the floor {on_floor}, maxima {[w[1] for w in want]}")
    assert on_floor[2] == 1.0 and want[2][1] == -10.0 and 0.05 <= on_floor[1] <= 0.25 and -7.0 < want[0][1] < -6.0
    if n_mels == 80:
        assert on_floor[0] == 0.0
    assert R.frame_classes(9000, 0) == (56, 54, 56)
    assert np.all(want[3][0][20:37] == -10.0) and not np.any(want[3][0][:20] == -10.0) and not np.any(want[3][0][37:] == -10.0)
    mel = make(n_mels, mode)
    results = [check_batch(mel, ("quiet", QUIET[i]), [c], 0, tol, mode != "f32", f"quiet {QUIET[i]} mels {n_mels} mode {mode}") for i, c in enumerate(clips)]
    fm, rows, g = check_batch(mel, "quiet", clips, 0, tol, mode != "f32", f"quiet, all four in one batch, mels {n_mels} mode {mode}")
    for i in range(len(clips)):
        assert same(fm[i], results[i][0][0]) and same(rows[i], results[i][1][0]) and g[i] == results[i][2][0]
        # what the code promises of the floor: no raw value under -10, no normalised value under the clip's clamp
        assert np.all(rows[i] >= np.float32(-10.0)) and g[i] >= np.float32(-10.0)
        lo = np.float32(np.float32(g[i]) - np.float32(8.0))
        assert np.all(fm[i] >= (lo + np.float32(4.0)) * np.float32(0.25))
    mel.close()
