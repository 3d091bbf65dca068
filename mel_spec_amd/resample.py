"""The stage in front of the frontends: PCM at 8-96 kHz, int16 or f32, resampled on the GPU to f32 PCM at the model rate
(include/melspec_resample.h: the definition -- torchaudio.functional.resample's default filter with integer arguments --, the conventions
and the statuses).  The output of the device calls stays in HBM, ready for the frontends' device calls on the same stream."""
from __future__ import annotations

import ctypes as C

import numpy as np

from ._lib import lib
from .hip import PCM_F32, PCM_S16, _check


def geometry(rate_in: int, rate_out: int):
    """(orig, new, width, max_inside_taps) of a rate pair; needs no device."""
    v = [C.c_uint32() for _ in range(4)]
    _check(lib().melspec_resample_geometry(rate_in, rate_out, *[C.byref(x) for x in v]))
    return tuple(int(x.value) for x in v)


def taps(rate_in: int, rate_out: int) -> np.ndarray:
    """The dense tap table, [new][2 * width + orig] f64; needs no device."""
    orig, new, width, _ = geometry(rate_in, rate_out)
    h = np.empty((new, 2 * width + orig), np.float64)
    _check(lib().melspec_resample_taps(rate_in, rate_out, h.ctypes.data_as(C.POINTER(C.c_double)), h.size))
    return h


def out_len(rate_in: int, rate_out: int, n_in: int) -> int:
    return int(lib().melspec_resample_out_len(rate_in, rate_out, n_in))


def _pcm(a):
    """(contiguous array, dtype code) of int16 or f32 samples"""
    a = np.asarray(a)
    if a.dtype == np.int16:
        return np.ascontiguousarray(a), PCM_S16
    return np.ascontiguousarray(a, dtype=np.float32), PCM_F32


def _code(pcm_dtype) -> int:
    if pcm_dtype in ("s16", "int16", np.int16) or (pcm_dtype == PCM_S16 and not isinstance(pcm_dtype, bool)):
        return PCM_S16
    if pcm_dtype is None or pcm_dtype in ("f32", np.float32) or pcm_dtype == PCM_F32:
        return PCM_F32
    raise ValueError(f"pcm_dtype must be 'f32' or 's16', not {pcm_dtype!r}")


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


class Resampler:
    """rate_in -> rate_out on one device (melspec_resampler_*)."""

    def __init__(self, rate_in: int, rate_out: int, device: int = -1):
        self._h = C.c_void_p()
        self.rate_in, self.rate_out = int(rate_in), int(rate_out)
        _check(lib().melspec_resampler_create(C.byref(self._h), device, self.rate_in, self.rate_out))

    @property
    def kernel_name(self) -> str:
        return lib().melspec_resampler_kernel_name(self._h).decode()

    def out_len(self, n_in: int) -> int:
        return out_len(self.rate_in, self.rate_out, n_in)

    def compute(self, samples) -> np.ndarray:
        """One clip, host memory in and out: int16 or f32 samples -> f32."""
        a, code = _pcm(samples)
        out = np.empty(self.out_len(a.size), np.float32)
        n = C.c_size_t()
        _check(lib().melspec_resample_host(self._h, a.ctypes.data_as(C.c_void_p), code, a.size, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)))
        return out[:n.value]

    def compute_uniform_device(self, d_pcm: int, pcm_dtype, clip_stride: int, clip_len: int, n_clips: int, d_out: int, out_stride: int, stream=None) -> None:
        """n_clips clips of clip_len samples in device memory -> out_len(clip_len) f32 samples each at d_out + i * out_stride; asynchronous."""
        _check(lib().melspec_resample_uniform_device(self._h, C.c_void_p(d_pcm), _code(pcm_dtype), clip_stride, clip_len, n_clips, C.c_void_p(d_out), out_stride, C.c_void_p(stream)))

    def compute_ragged_device(self, d_pcm: int, pcm_dtype, offsets, lengths, d_out: int, out_offsets=None, stream=None) -> None:
        """Clip i: lengths[i] samples at d_pcm + offsets[i] -> d_out + out_offsets[i] (None: packed in clip order); asynchronous."""
        off, off_p = _u64(offsets)
        ln, ln_p = _u64(lengths)
        assert off.size == ln.size
        oo_p = None
        if out_offsets is not None:
            oo, oo_p = _u64(out_offsets)
            assert oo.size == off.size
        _check(lib().melspec_resample_ragged_device(self._h, C.c_void_p(d_pcm), _code(pcm_dtype), off_p, ln_p, off.size, C.c_void_p(d_out), oo_p, C.c_void_p(stream)))

    def synchronize(self, stream=None) -> None:
        _check(lib().melspec_resampler_synchronize(self._h, C.c_void_p(stream)))

    def close(self) -> None:
        if self._h is not None and self._h.value:
            lib().melspec_resampler_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
