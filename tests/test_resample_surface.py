"""The resampler's surface (include/melspec_resample.h) and what needs no GPU: every symbol declared once, exported, in
_lib.RESAMPLE_SIGNATURES with the same argument count, used by melspec_resample.hpp, declared in resample.rs, and in neither
melspec_hip.h nor _lib.SIGNATURES; the header is C99; the verdicts on a NULL handle and on bad arguments; the geometry, out_len and the
tap table against the model of tests/resample_ref.py; and the model's own sanity.  The GPU side: tests/test_resample.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resample_ref as R
from conftest import ROOT

SYMBOLS = {
    "melspec_resample_geometry": 6,
    "melspec_resample_taps": 4,
    "melspec_resample_out_len": 3,
    "melspec_resampler_create": 4,
    "melspec_resampler_destroy": 1,
    "melspec_resampler_kernel_name": 1,
    "melspec_resample_uniform_device": 9,
    "melspec_resample_ragged_device": 9,
    "melspec_resample_host": 7,
    "melspec_resampler_synchronize": 2,
}
# rate_in, rate_out, then for the five tabulated pairs orig, new, width, K, inside taps per phase (min, max)
TABLE = {(48000, 16000): (3, 1, 19, 41, 37, 37), (44100, 16000): (441, 160, 17, 475, 33, 34), (8000, 16000): (1, 2, 7, 15, 12, 13),
         (22050, 16000): (441, 320, 9, 459, 16, 17), (24000, 16000): (3, 2, 10, 23, 18, 19)}
PAIRS = sorted(TABLE) + [(32000, 16000), (11025, 16000), (96000, 16000), (16000, 24000)]


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as fh:
        return fh.read()


def _args(text, pattern):
    """the argument count of the one declaration `pattern(...)` finds"""
    m = re.findall(pattern + r"\(([^()]*)\)", text)
    assert len(m) == 1, (pattern, len(m))
    return len([a for a in m[0].split(",") if a.strip()])


def _code(text):
    """a C header without its comments"""
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@pytest.mark.parametrize("name", sorted(SYMBOLS))
def test_symbol_everywhere(name):
    from mel_spec_amd import _lib
    want = SYMBOLS[name]
    assert _args(_code(_read("include", "melspec_resample.h")), r"\b" + name) == want
    assert len(_lib.RESAMPLE_SIGNATURES[name][1]) == want
    assert getattr(_lib.lib(), name) is not None
    assert getattr(_lib.lib(), name).argtypes is not None, "lib() did not apply RESAMPLE_SIGNATURES"
    assert re.search(r"\b" + name + r"\(", _read("include", "melspec_resample.hpp")), "not used by melspec_resample.hpp"
    assert _args(_read("mel_spec_amd", "rust", "resample.rs"), r"\bfn " + name) == want, "resample.rs declares it with another argument count"
    assert name not in _lib.SIGNATURES
    assert not re.search(r"\b" + name + r"\b", _read("include", "melspec_hip.h"))
    assert not re.search(r"\b" + name + r"\b", _read("mel_spec_amd", "rust", "hip.rs"))


def test_header_is_c99_and_complete():
    from mel_spec_amd import _lib
    import mel_spec_amd
    hdr = _read("include", "melspec_resample.h")
    declared = re.findall(r"\b(melspec_resampl\w+)\s*\(", _code(hdr))
    assert sorted(declared) == sorted(SYMBOLS), declared
    assert sorted(_lib.RESAMPLE_SIGNATURES) == sorted(SYMBOLS)
    assert "melspec_resampler" not in _read("include", "melspec_hip.h")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-fsyntax-only", "-x", "c", os.path.join(ROOT, "include", "melspec_resample.h")])
    assert _lib.lib().melspec_abi_version() == 1
    for scope in ("device memory", "streaming", "16-bit output", "widths or rolloffs", "sharded"):
        assert scope in hdr, f"the header comment does not state that '{scope}' is out of scope"
    assert mel_spec_amd.Resampler is mel_spec_amd.resample.Resampler and "Resampler" in mel_spec_amd.__all__
    for attr in ("out_len", "compute", "compute_uniform_device", "compute_ragged_device", "synchronize"):
        assert callable(getattr(mel_spec_amd.Resampler, attr)), attr
    assert callable(mel_spec_amd.resample.geometry) and callable(mel_spec_amd.resample.taps)


def test_verdicts_need_no_device():
    from mel_spec_amd import _lib
    L = _lib.lib()
    buf = np.full(1024, 7.0, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    u = np.zeros(4, np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    n = C.c_size_t(99)
    for rc in (L.melspec_resample_uniform_device(None, p, 0, 16, 16, 1, p, 16, None),
               L.melspec_resample_uniform_device(None, p, 7, 16, 16, 1, p, 16, None),      # the NULL handle comes before the dtype
               L.melspec_resample_ragged_device(None, p, 1, u, u, 1, p, None, None),
               L.melspec_resample_host(None, p, 0, 16, p, 16, C.byref(n)),
               L.melspec_resampler_synchronize(None, None)):
        assert rc == _lib.ERR_INVALID_ARG and "NULL" in _lib.last_error()
    assert n.value == 99 and np.all(buf == 7.0)
    L.melspec_resampler_destroy(None)
    assert L.melspec_resampler_kernel_name(None) == b""
    # the arguments of create are checked before a device is looked for
    h = C.c_void_p(5)
    assert L.melspec_resampler_create(None, -1, 48000, 16000) == _lib.ERR_INVALID_ARG
    for rate_in, rate_out, want in ((0, 16000, _lib.ERR_INVALID_ARG), (48000, 0, _lib.ERR_INVALID_ARG), (4097, 1, _lib.ERR_UNSUPPORTED), (16000, 16001, _lib.ERR_UNSUPPORTED)):
        assert L.melspec_resampler_create(C.byref(h), -1, rate_in, rate_out) == want and not h.value
        h = C.c_void_p(5)
        assert L.melspec_resample_geometry(rate_in, rate_out, None, None, None, None) == want
        assert L.melspec_resample_taps(rate_in, rate_out, buf.ctypes.data_as(C.POINTER(C.c_double)), 512) == want
    assert L.melspec_resample_out_len(0, 16000, 100) == 0 and L.melspec_resample_out_len(16000, 0, 100) == 0
    assert L.melspec_resample_geometry(8192, 2, None, None, None, None) == _lib.OK          # 4096 : 1
    d = np.full(64, 7.0)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    assert L.melspec_resample_taps(48000, 16000, None, 41) == _lib.ERR_INVALID_ARG
    assert L.melspec_resample_taps(48000, 16000, dp, 40) == _lib.ERR_CAPACITY and np.all(d == 7.0)
    assert L.melspec_resample_taps(48000, 16000, dp, 41) == _lib.OK and np.all(d[41:] == 7.0)
    assert np.all(buf == 7.0)


@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_geometry_out_len_and_taps(pair):
    from mel_spec_amd import resample
    rate_in, rate_out = pair
    orig, new, width, K, M, m_ = R.geometry(rate_in, rate_out)
    ins = R.inside(rate_in, rate_out)
    got = resample.geometry(rate_in, rate_out)
    assert got == (orig, new, width, int(ins.sum(axis=1).max()))
    if pair in TABLE:
        assert (orig, new, width, K, int(ins.sum(axis=1).min()), got[3]) == TABLE[pair]
    for n in (0, 1, orig - 1, orig, orig + 1, 10 ** 6 + 1):
        assert resample.out_len(rate_in, rate_out, n) == -((-new * n) // orig) == R.out_len(rate_in, rate_out, n)
    h, want = resample.taps(rate_in, rate_out), R.taps(rate_in, rate_out)
    assert h.shape == want.shape == (new, K)
    assert np.all(h[~ins] == 0.0) and not np.any(np.signbit(h[~ins])), "outside taps are exactly 0.0"
    assert float(np.abs(h - want)[ins].max()) <= 2.0 ** -49
    for p in range(new):
        ks = np.nonzero(ins[p])[0]
        assert np.all(np.diff(ks) == 1), "the inside taps of a phase are contiguous"


# ---- the model alone ----
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_model_row_sums(pair):
    sums = R.taps(*pair).sum(axis=1)
    assert 1.0000 <= sums.min() and sums.max() <= 1.0010, (sums.min(), sums.max())


def test_model_sine():
    n = 4800
    x = np.sin(2 * np.pi * 440.0 * np.arange(n) / 48000.0)
    y = R.resample(x, 48000, 16000)
    want = np.sin(2 * np.pi * 440.0 * np.arange(y.size) / 16000.0)
    err = float(np.abs(y - want)[20:-20].max())
    assert y.size == 1600 and err <= 1e-3, err


@pytest.mark.parametrize("pair", [(48000, 16000), (44100, 16000), (8000, 16000), (16000, 24000)], ids=lambda p: f"{p[0]}-{p[1]}")
def test_model_shift_invariance(pair):
    orig, new = R.geometry(*pair)[:2]
    x = (np.random.default_rng(5).standard_normal(3 * orig + 700) * 0.3).astype(np.float32)
    y = R.resample(x, *pair)
    ys = R.resample(np.concatenate([np.zeros(orig, np.float32), x]), *pair)
    assert ys.size == y.size + new
    assert np.array_equal(ys[new:].view(np.uint64), y.view(np.uint64)), "a shift by orig samples is a shift by new outputs, bit for bit"
    # (the first `new` outputs see the clip's head through the filter's tail: they are not zero, only small)
    assert np.all(np.abs(ys[:new]) <= np.abs(x).max())
