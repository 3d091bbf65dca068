"""The numpy f64 model of the resampler's definition (include/melspec_resample.h), written from that text and not from the library:
torchaudio.functional.resample's default filter (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) with integer arguments.

  geometry(rate_in, rate_out) -> orig, new, width, K, M, m_
  inside(rate_in, rate_out)   -> bool [new][K]
  taps(rate_in, rate_out)     -> f64 [new][K], outside taps exactly 0
  out_len(rate_in, rate_out, n)
  resample(x, rate_in, rate_out, bounds=False) -> y f64 (the sum over the inside taps in ascending k, unrounded); with bounds also
      A = sum |h_k x_k|, X = sum |x_k| and the number of inside taps, per output
An int16 input has the values s * 2^-15.  rate_in == rate_out is the converted input."""
from math import gcd

import numpy as np


def geometry(rate_in, rate_out):
    g = gcd(rate_in, rate_out)
    orig, new = rate_in // g, rate_out // g
    M, m_ = max(orig, new), min(orig, new)
    width = -((-600 * orig) // (99 * m_))
    return orig, new, width, 2 * width + orig, M, m_


def _m(rate_in, rate_out):
    orig, new, width, K, M, m_ = geometry(rate_in, rate_out)
    k = np.arange(K, dtype=np.int64)[None, :]
    p = np.arange(new, dtype=np.int64)[:, None]
    return (k - width) * new - p * orig


def inside(rate_in, rate_out):
    M = geometry(rate_in, rate_out)[4]
    return 99 * np.abs(_m(rate_in, rate_out)) < 600 * M


def taps(rate_in, rate_out):
    orig, new, width, K, M, m_ = geometry(rate_in, rate_out)
    m = _m(rate_in, rate_out)
    t = (99.0 * m.astype(np.float64)) / (100.0 * float(M))
    a = np.pi * t
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(m == 0, 1.0, np.sin(a) / a)
    h = sinc * np.cos(a / 12.0) ** 2 * ((99.0 * float(m_)) / (100.0 * float(orig)))
    return np.where(inside(rate_in, rate_out), h, 0.0)


def out_len(rate_in, rate_out, n):
    orig, new = geometry(rate_in, rate_out)[:2]
    return -((-new * int(n)) // orig)


def values(x):
    """the samples as f64: int16 is s * 2^-15"""
    x = np.asarray(x)
    return x.astype(np.float64) / 32768.0 if x.dtype == np.int16 else x.astype(np.float64)


def resample(x, rate_in, rate_out, bounds=False):
    v = values(x)
    L = v.size
    n_out = out_len(rate_in, rate_out, L)
    if rate_in == rate_out:
        return (v, np.abs(v), np.abs(v), np.ones(L, np.int64)) if bounds else v
    orig, new, width, K, M, m_ = geometry(rate_in, rate_out)
    h, ins = taps(rate_in, rate_out), inside(rate_in, rate_out)
    blocks = -(-n_out // new) if n_out else 0
    xp = np.zeros(width + (blocks + 1) * orig + width + K)
    xp[width:width + L] = v
    j = np.arange(blocks)
    y = np.zeros((blocks, new))
    A = np.zeros((blocks, new))
    X = np.zeros((blocks, new))
    for p in range(new):
        ks = np.nonzero(ins[p])[0]
        assert ks.size and np.all(np.diff(ks) == 1), "the inside taps of a phase are contiguous"
        acc = np.zeros(blocks)
        a = np.zeros(blocks)
        s = np.zeros(blocks)
        with np.errstate(invalid="ignore", over="ignore"):
            for k in ks:                      # ascending k
                xk = xp[j * orig + k]         # x[j orig + k - width]
                acc = acc + h[p, k] * xk
                a += np.abs(h[p, k] * xk)
                s += np.abs(xk)
        y[:, p], A[:, p], X[:, p] = acc, a, s
    n_in = np.broadcast_to(ins.sum(axis=1)[None, :], (blocks, new)).reshape(-1)[:n_out]
    y, A, X = y.reshape(-1)[:n_out], A.reshape(-1)[:n_out], X.reshape(-1)[:n_out]
    return (y, A, X, n_in) if bounds else y


def tolerance(y, A, X, n_in):
    """|y_gpu - y| may be: one rounding to f32 + the f64 summation bound in any order, fused or not + the 2^-49 tap allowance + a flushed
    subnormal"""
    half = 0.5 * np.spacing(np.abs(y).astype(np.float32)).astype(np.float64)
    return half + n_in * 2.0 ** -52 * A + 2.0 ** -49 * X + 2.0 ** -126
