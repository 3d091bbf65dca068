"""The surface of the centred Whisper features with int16 PCM in / f16, bf16 out: every melspec_whisper_*_io symbol is declared in
include/melspec_hip.h, exported by the built library and listed by mel_spec_amd/_lib.py with the same number of arguments; the Python
package has the functions; the header no longer lists the 16-bit ends as uncovered; the ABI version is 1; and the conversion contract the
GPU tests' exact yardsticks rest on holds on the CPU (int16 -> f32 is exact; numpy's and torch's roundings to f16 / bf16 are to nearest
even).  The arithmetic of the calls' arguments and of the 16-byte store rule: tests/cpp/whisper_centered_io_host.cpp, built and run here.
No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT

SYMBOLS = {           # name -> arguments
    "melspec_whisper_supports_io": 3,
    "melspec_whisper_compute_uniform_device_io": 11,
    "melspec_whisper_compute_ragged_device_io": 12,
    "melspec_whisper_compute_uniform_device_split_io": 11,
    "melspec_whisper_compute_ragged_device_split_io": 12,
    "melspec_whisper_compute_host_io": 10,
}


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
    assert len(_lib.SIGNATURES[name][1]) == want
    assert getattr(_lib.lib(), name) is not None
    assert name in _read("INTEGRATION.md")


def test_header_and_abi():
    from mel_spec_amd import _lib
    hdr = _read("include", "melspec_hip.h")
    assert not re.search(r"NOT covered[^.]*int16", hdr), "the header still lists the 16-bit ends of the Whisper calls as uncovered"
    assert re.search(r"NOT covered[^.]*_desc", hdr), "the device-resident clip table is still uncovered and the header says so"
    assert _lib.lib().melspec_abi_version() == 1
    # a NULL context and unknown dtype codes are answered without a device
    L = _lib.lib()
    assert L.melspec_whisper_supports_io(None, 1, 1) == 0
    assert L.melspec_whisper_compute_uniform_device_io(None, None, 1, 0, 0, 1, 0, None, 1, 0, None) == _lib.ERR_INVALID_ARG and "NULL" in _lib.last_error()
    assert L.melspec_whisper_compute_host_io(None, None, 1, 0, 0, None, 1, 0, 0, None) == _lib.ERR_INVALID_ARG and "NULL" in _lib.last_error()


def test_python_functions():
    import mel_spec_amd
    for m in ("supports_whisper_io", "whisper_uniform_device_io", "whisper_ragged_device_io", "whisper_uniform_device_split_io", "whisper_ragged_device_split_io",
              "whisper_features_io", "whisper_features_batch_io", "whisper_split_io"):
        assert callable(getattr(mel_spec_amd, m)) and m in mel_spec_amd.__all__, m


def test_conversion_contract():
    """int16 * 2^-15 is exact in f32 for every int16; astype(float16) and torch's .to(bfloat16) round to nearest, ties to even; -10 (a silent
    raw row) is representable in both 16-bit types"""
    v = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    f = v.astype(np.float32) * np.float32(2.0 ** -15)
    assert np.array_equal(f.astype(np.float64) * 32768.0, v.astype(np.float64))
    # ties: f16 has 10 fraction bits, bf16 has 7 -- 1 + (2 k + 1) ulp / 2 lies halfway and goes to the even neighbour
    for k in range(4):
        tie16 = np.array([1.0 + (2 * k + 1) * 2.0 ** -11], np.float32)
        assert tie16.astype(np.float16)[0] == np.float16(1.0 + 2 * ((k + 1) // 2) * 2.0 ** -10)
        tie_b = torch.tensor([1.0 + (2 * k + 1) * 2.0 ** -8], dtype=torch.float32)
        assert float(tie_b.to(torch.bfloat16)[0]) == 1.0 + 2 * ((k + 1) // 2) * 2.0 ** -7
    just_above = np.array([1.0 + 2.0 ** -11 + 2.0 ** -23], np.float32)
    assert just_above.astype(np.float16)[0] == np.float16(1.0 + 2.0 ** -10)
    assert float(torch.tensor([1.0 + 2.0 ** -8 + 2.0 ** -23]).to(torch.bfloat16)[0]) == 1.0 + 2.0 ** -7
    assert np.float32(-10.0).astype(np.float16) == -10.0 and float(torch.tensor([-10.0]).to(torch.bfloat16)[0]) == -10.0
    # monotone: the rounded maximum is the maximum of the rounded values
    x = np.random.default_rng(7).uniform(-10.0, 4.0, 4096).astype(np.float32)
    assert x.astype(np.float16).max() == np.float32(x.max()).astype(np.float16)
    xb = torch.from_numpy(x).to(torch.bfloat16)
    assert float(xb.max()) == float(torch.tensor([x.max()]).to(torch.bfloat16)[0])


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_whisper_centered_io_host(tmp_path, sanitize):
    exe = tmp_path / "whisper_centered_io_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "whisper_centered_io_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("whisper_centered_io_host: ok"), p.stdout + p.stderr
