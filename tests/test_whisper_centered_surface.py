"""The surface of the centred Whisper features: every melspec_whisper_* symbol is declared in include/melspec_hip.h, used by
include/melspec_hip.hpp, declared by mel_spec_amd/rust/hip.rs and listed by mel_spec_amd/_lib.py with the same number of arguments, the
Python package has the functions (module-level: the frontend classes' attributes are a pinned set), and melspec_whisper_num_frames through the library equals the reference helper.  No GPU."""
import os
import re

import pytest

from conftest import ROOT
import whisper_centered_ref as R

SYMBOLS = {           # name -> arguments
    "melspec_whisper_supports": 1,
    "melspec_whisper_num_frames": 3,
    "melspec_whisper_kernel_name": 1,
    "melspec_whisper_compute_uniform_device": 9,
    "melspec_whisper_compute_ragged_device": 10,
    "melspec_whisper_compute_uniform_device_split": 9,
    "melspec_whisper_compute_ragged_device_split": 10,
    "melspec_whisper_compute_host": 8,
}
PLAIN = [399, 400, 401, 559, 560, 599, 600, 639, 640, 679, 680, 1119, 1120]
PADDED = [0, 1, 199, 200, 201, 399, 400, 4599, 4600, 4601, 4799, 4800, 4801, 9000]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _args(text, pattern):
    """the argument count of the one declaration `pattern(...)` finds"""
    m = re.findall(pattern + r"\(([^()]*)\)", text)
    assert len(m) == 1, (pattern, len(m))
    return len([a for a in m[0].split(",") if a.strip()])


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_everywhere(name):
    from mel_spec_amd import _lib
    want = SYMBOLS[name]
    assert _args(_read("include", "melspec_hip.h"), r"\b" + name) == want
    assert _args(_read("mel_spec_amd", "rust", "hip.rs"), r"fn " + name) == want
    assert len(_lib.SIGNATURES[name][1]) == want
    assert re.search(r"\b" + name + r"\(", _read("include", "melspec_hip.hpp")), "not used by melspec_hip.hpp"
    assert getattr(_lib.lib(), name) is not None
    assert name in _read("INTEGRATION.md")


def test_python_methods():
    import mel_spec_amd
    for m in ("whisper_num_frames", "whisper_features", "whisper_features_batch", "whisper_split", "whisper_uniform_device", "whisper_ragged_device",
              "whisper_uniform_device_split", "whisper_ragged_device_split", "whisper_kernel_name", "supports_whisper"):
        assert callable(getattr(mel_spec_amd, m)), m


def test_num_frames_constants():
    """the helper's own frame counts (the GPU test of the library's is test_whisper_centered.py::test_num_frames)"""
    assert [R.num_frames(n, 0) for n in PLAIN] == [0, 2, 2, 3, 3, 3, 3, 3, 4, 4, 4, 6, 7]
    assert [R.num_frames(n, 4800) for n in PADDED] == [30] * len(PADDED)
    assert R.num_frames(176000, 0) == 1100 and R.num_frames(176000, 480000) == 3000
