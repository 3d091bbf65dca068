"""The reference the GPU tests of the centred Whisper features rest on (tests/whisper_centered_ref.py: reflect pad + the oracle's STFT, mel
bank and log10 + the clip-wide clamp in f64) against an independent implementation: the openai-whisper recipe written in torch f64 --
torch.stft(center=True) with the periodic Hann window, [..., :-1], filters @ |X|^2, clamp(1e-10).log10(), maximum(max - 8), (x + 4) / 4.
Live, on JFK and on the four-tone fixture, at both pad_to values; gate 1e-9."""
import numpy as np
import pytest
import torch

import whisper_centered_ref as R


def torch_recipe(x, pad_to, n_mels):
    s = torch.from_numpy(R.signal(x, pad_to).astype(np.float64))
    window = torch.hann_window(R.N_FFT, periodic=True, dtype=torch.float64)
    stft = torch.stft(s, R.N_FFT, R.HOP, window=window, center=True, pad_mode="reflect", return_complex=True)
    mag = stft[..., :-1].abs() ** 2
    mel = torch.from_numpy(R.filters(n_mels)) @ mag
    log = torch.clamp(mel, min=1e-10).log10()
    log = torch.maximum(log, log.max() - 8.0)
    return ((log + 4.0) / 4.0).numpy()          # [n_mels][T]


@pytest.mark.parametrize("pad_to", [0, 480000])
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("which", ["jfk", "four_tone"])
def test_reference_against_torch(which, n_mels, pad_to, jfk, four_tone):
    x = jfk if which == "jfk" else four_tone
    _, _, want = R.features(x, pad_to, n_mels)
    got = torch_recipe(x, pad_to, n_mels)
    T = R.num_frames(x.shape[0], pad_to)
    assert want.shape == (T, n_mels) and got.shape == (n_mels, T)
    if pad_to:
        assert T == 3000
    elif which == "jfk":
        assert T == 1100
    d = float(np.abs(got.T - want).max())
    print(f"{which} n_mels {n_mels} pad_to {pad_to}: T {T}, max |reference - torch f64| = {d:.3e}")
    assert d <= 1e-9


def test_silent_frames_of_jfk(jfk):
    """JFK under pad_to = 480000: 3000 frames, 1902 of them on the floor in every band -- the 1898 that lie wholly in the zero extension
    (frame t reads s[160 t - 200 ..), so from t = ceil((n + 200) / 160) on) and the clip's last four, which are below 1e-10 by themselves"""
    raw = R.raw_rows(jfk, 480000, 80)
    first_silent = -(-(jfk.shape[0] + R.PAD) // R.HOP)
    assert raw.shape[0] == 3000 and first_silent == 1102
    assert np.all(raw[first_silent:] == R.FLOOR)
    assert int((raw == R.FLOOR).all(axis=1).sum()) == 1902
