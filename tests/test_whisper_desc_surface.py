"""The centred Whisper features from a clip table in device memory (melspec_whisper_compute_ragged_device_desc*): what needs no GPU.  Every
symbol is declared once in the header with its argument count, exported by the built library, in the ctypes table with the same count,
used by the C++ wrapper, bound in the Rust shim and named in INTEGRATION.md; the Python functions are module-level; a NULL context is
answered without a device; and the planner's host half (mel_spec_amd/csrc/whisper_centered_plan.hpp: wc_desc_*, wc_args_desc*) runs
as a stand-alone program, plain and with -fsanitize=address,undefined (tests/cpp/whisper_desc_plan_host.cpp).  The GPU side:
tests/test_whisper_desc.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

SYMBOLS = {
    "melspec_whisper_supports_desc": 1,
    "melspec_whisper_compute_ragged_device_desc": 10,
    "melspec_whisper_compute_ragged_device_desc_split": 10,
    "melspec_whisper_compute_ragged_device_desc_io": 12,
    "melspec_whisper_compute_ragged_device_desc_split_io": 12,
}
PYTHON = ["supports_whisper_desc", "whisper_ragged_device_desc", "whisper_ragged_device_desc_split", "whisper_ragged_device_desc_io", "whisper_ragged_device_desc_split_io"]


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
    assert re.search(r"\b" + name + r"\(", _read("include", "melspec_hip.hpp")), "not used by melspec_hip.hpp"
    shim = _read("mel_spec_amd", "rust", "hip.rs")
    assert _args(shim, r"\bfn " + name) == want, "hip.rs binds it with another argument count"
    assert len(re.findall(r"\b" + name + r"\(", shim)) == 2, "hip.rs: one declaration, one call from a thin unsafe fn"
    assert name in _read("INTEGRATION.md")


def test_header_abi_and_python():
    from mel_spec_amd import _lib
    import mel_spec_amd
    hdr = _read("include", "melspec_hip.h")
    notes = re.findall(r"NOT covered[^.]*\.", hdr)
    assert len(notes) == 2 and all("_desc" in n and "pad_to == 0" in n for n in notes), notes
    assert _lib.lib().melspec_abi_version() == 1
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "melspec_hip.h")])
    for name in PYTHON:
        assert callable(getattr(mel_spec_amd, name)) and name in mel_spec_amd.__all__, name
        assert not hasattr(mel_spec_amd.HipMelSpectrogram, name), "a function: the classes' attributes are a pinned set"
    import inspect
    for name in PYTHON[1:]:
        p = inspect.signature(getattr(mel_spec_amd, name)).parameters
        assert p["pad_to"].default == 480000 and ("mel_major" not in p or p["mel_major"].default is True), name


def test_null_context_needs_no_device():
    from mel_spec_amd import _lib
    L = _lib.lib()
    buf = np.zeros(1024, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert L.melspec_whisper_supports_desc(None) == 0
    for rc in (L.melspec_whisper_compute_ragged_device_desc(None, p, p, p, 1, 4800, p, None, 1, None),
               L.melspec_whisper_compute_ragged_device_desc(None, None, None, None, 0, 0, None, None, 1, None),
               L.melspec_whisper_compute_ragged_device_desc_split(None, p, p, p, 1, 4800, p, None, p, None),
               L.melspec_whisper_compute_ragged_device_desc_io(None, p, 7, p, p, 1, 4800, p, 9, None, 1, None),
               L.melspec_whisper_compute_ragged_device_desc_split_io(None, p, 1, p, p, 1, 4800, p, 1, None, p, None)):
        assert rc == _lib.ERR_INVALID_ARG and "NULL" in _lib.last_error()
    assert np.all(buf == 0)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_desc_plan_on_the_host(tmp_path, sanitize):
    exe = tmp_path / "whisper_desc_plan_host"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "mel_spec_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "whisper_desc_plan_host.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith("whisper_desc_plan_host: ok"), p.stdout + p.stderr
