"""The reference of the centred Whisper features (melspec_whisper_*), composed from the oracle's own pieces and kept beside the tests:
numpy.pad(s, 200, mode="reflect") -> oracle.compute_all_cpu(.., 400, 160)[:-1] -> oracle.log_mel_spectrogram(S, mel_filterbank(16000, 400,
n_mels)) -> the clip maximum and (max(x, g - 8) + 4) / 4 in f64.  tests/test_whisper_centered_ref.py pins it to the openai-whisper recipe
written in torch f64; the GPU tests rest on it."""
import functools

import numpy as np

from oracle import oracle as O

N_FFT, HOP, PAD = 400, 160, 200
FLOOR = -10.0


def signal(x, pad_to: int) -> np.ndarray:
    """step 1: the clip as it is (pad_to == 0), or trimmed / zero-extended to pad_to samples"""
    x = np.asarray(x, np.float32).reshape(-1)
    if pad_to == 0:
        return x
    s = np.zeros(pad_to, np.float32)
    n = min(x.shape[0], pad_to)
    s[:n] = x[:n]
    return s


def num_frames(n: int, pad_to: int) -> int:
    P = pad_to if pad_to else n
    return 0 if P < N_FFT else P // HOP


def frame_classes(n: int, pad_to: int):
    """(T, interior, first_silent): frames [0, 2) and [2 + interior, first_silent) read mirrored samples or straddle the end of the
    caller's samples (the library's edge frames), [2, 2 + interior) are ordinary un-centred frames, [first_silent, T) read zeros only --
    the rule of the library's host plan (wc_clip), restated"""
    P = pad_to if pad_to else n
    n_eff = min(n, P)
    T = 0 if P < N_FFT else P // HOP
    if T == 0 or n_eff == 0:
        return T, 0, 0
    t_max = (n_eff - PAD) // HOP if n_eff >= PAD else 0
    interior = t_max - 1 if t_max >= 2 else 0
    return T, interior, min(max(-(-(n_eff + PAD) // HOP), 2), T)


@functools.lru_cache(maxsize=None)
def filters(n_mels: int) -> np.ndarray:
    return O.mel_filterbank(16000.0, N_FFT, n_mels)


def _spectra(s: np.ndarray) -> np.ndarray:
    r = np.pad(s.astype(np.float32), PAD, mode="reflect")
    return O.compute_all_cpu(r, N_FFT, HOP)[:-1]


def raw_rows(x, pad_to: int, n_mels: int) -> np.ndarray:
    """steps 1-4: [T][n_mels] f64, log10(max(E, 1e-10))"""
    s = signal(x, pad_to)
    T = num_frames(s.shape[0], 0)
    if T == 0:
        return np.zeros((0, n_mels))
    raw = O.log_mel_spectrogram(_spectra(s), filters(n_mels))
    assert raw.shape == (T, n_mels), (raw.shape, T)
    return raw


def raw_rows_many(clips, pad_to: int, n_mels: int) -> list:
    """raw_rows of many clips with one pass through the filterbank"""
    sigs = [signal(x, pad_to) for x in clips]
    Ts = [num_frames(s.shape[0], 0) for s in sigs]
    spec = [_spectra(s) for s, T in zip(sigs, Ts) if T]
    if not spec:
        return [np.zeros((0, n_mels)) for _ in clips]
    allraw = O.log_mel_spectrogram(np.concatenate(spec), filters(n_mels))
    out, cur = [], 0
    for T in Ts:
        out.append(allraw[cur:cur + T])
        cur += T
    return out


def normalise(raw: np.ndarray):
    """steps 5-6 in f64: (g, [T][n_mels])"""
    g = float(raw.max()) if raw.size else FLOOR
    return g, (np.maximum(raw, g - 8.0) + 4.0) / 4.0


def features(x, pad_to: int, n_mels: int):
    """(raw [T][n_mels], g, normalised [T][n_mels]), all f64"""
    raw = raw_rows(x, pad_to, n_mels)
    g, out = normalise(raw)
    return raw, g, out


def fold_f32(rows: np.ndarray, g) -> np.ndarray:
    """step 6 as the finalise pass does it, in f32: what a consumer of the split output computes"""
    rows = np.asarray(rows, np.float32)
    lo = np.float32(np.float32(g) - np.float32(8.0))
    return (np.maximum(rows, lo) + np.float32(4.0)) * np.float32(0.25)
