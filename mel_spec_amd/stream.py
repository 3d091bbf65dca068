"""Streaming side of the reference over the C ABI (melspec_stream_*): a bank of live streams whose
overlap-save state lives in HBM, and a single-stream `RingBuffer` with the reference's method names
(src/rb.rs:18-121: add_frame / add / maybe_mel)."""
import ctypes as C
from collections import deque
from typing import List, Optional, Sequence

import numpy as np

from ._lib import lib
from .hip import PCM_F32, PCM_S16, _OUT_NUMPY, HipMelSpectrogram, _check, _f32, _fp, _out_code
from .vad import DetectionSettings, VadFrameTiming, VoiceActivity

# melspec_vad_activity (include/melspec_hip.h): one 8-byte record per emitted frame
ACTIVITY_DTYPE = np.dtype([("valid", "u1"), ("active", "u1"), ("leading_active_columns", "<u2"), ("active_columns", "<u2"),
                           ("window_columns", "<u2")])

_u32p = C.POINTER(C.c_uint32)


def _u32(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint32)


class _Bank:
    """What the banks of live streams share: the handle's life, and the calls that differ by the C symbols' prefix (_P) only."""
    _P = ""

    def _fn(self, name: str):
        return getattr(lib(), self._P + name)

    def close(self) -> None:
        if getattr(self, "_h", None):
            self._fn("destroy")(self._h)
            self._h = None

    __del__ = close

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        if ids is None:
            _check(self._fn("reset")(self._h, None, 0))
        else:
            a = _u32(ids)
            _check(self._fn("reset")(self._h, a.ctypes.data_as(_u32p), a.shape[0]))

    def frames_after(self, stream: int, n_new: int) -> int:
        return int(self._fn("frames_after")(self._h, stream, n_new))

    def input_ptr(self, stream: int) -> int:
        return int(self._fn("input_ptr")(self._h, stream) or 0)

    def _collect(self, out: np.ndarray, frames: np.ndarray, cap: Optional[int] = None) -> List[np.ndarray]:
        assert cap is None or int(frames.sum()) == cap
        res, cur = [], 0
        for f in frames:
            res.append(out[cur:cur + int(f)])
            cur += int(f)
        return res

    @staticmethod
    def _dev(ids: Sequence[int], lens: Sequence[int], *offsets):
        """a device push's arguments: (frames to fill, n, the pointers of ids, lens and each optional list of uint64 offsets, the arrays)"""
        arrs = [_u32(ids), _u32(lens)] + [None if o is None else np.ascontiguousarray(o, np.uint64) for o in offsets]
        ptrs = [None if x is None else x.ctypes.data_as(C.POINTER(C.c_uint64) if x.dtype == np.uint64 else _u32p) for x in arrs]
        return np.zeros(arrs[0].shape[0], np.uint32), arrs[0].shape[0], ptrs, arrs

    def _gather(self, ids: Sequence[int], chunks: Sequence, allow_s16: bool):
        """a push's arguments: (ids, PCM code, the chunks back to back, their lengths, rows the push will emit, a frames array to fill)"""
        a = _u32(ids)
        arrs = [np.asarray(c) for c in chunks]
        assert len(arrs) == a.shape[0]
        s16 = [allow_s16 and x.dtype == np.int16 for x in arrs]
        if any(s16) and not all(s16):
            raise ValueError("all chunks of one push must have the same dtype (np.int16, or float)")
        pcm = PCM_S16 if arrs and all(s16) else PCM_F32
        xs = [np.ascontiguousarray(x).ravel() if pcm == PCM_S16 else _f32(x).ravel() for x in arrs]
        lens = _u32([x.shape[0] for x in xs])
        flat = np.concatenate(xs) if xs else np.zeros(0, np.float32)
        cap = sum(self.frames_after(int(s), int(n)) for s, n in zip(a, lens))
        return a, pcm, flat, lens, cap, np.zeros(a.shape[0], np.uint32)


class StreamBank(_Bank):
    """n_streams independent Spectrogram::add states (src/stft.rs:48-86) on one HipMelSpectrogram's geometry."""
    _P = "melspec_stream_"

    def __init__(self, mel: HipMelSpectrogram, n_streams: int, max_chunk: int):
        self._mel = mel                      # keeps the ctx alive
        self.n_streams, self.max_chunk, self.n_mels = int(n_streams), int(max_chunk), mel.n_mels
        h = C.c_void_p()
        _check(lib().melspec_stream_create(C.byref(h), mel._h, self.n_streams, self.max_chunk), construct=True)
        self._h = h

    def _flush_args(self, ids: Sequence[int], dtype=np.float32):
        a = _u32(ids)
        return a, np.empty((a.shape[0], self.n_mels), dtype), np.zeros(a.shape[0], np.uint32)

    def push(self, ids: Sequence[int], chunks: Sequence) -> List[np.ndarray]:
        """Append chunks[i] (any length <= max_chunk) to stream ids[i]; returns the frames each stream emitted, [k_i, n_mels]."""
        a, _, flat, lens, cap, frames = self._gather(ids, chunks, False)
        out = np.empty((cap, self.n_mels), np.float32)
        _check(lib().melspec_stream_push_host(self._h, a.ctypes.data_as(_u32p), _fp(flat), lens.ctypes.data_as(_u32p), a.shape[0],
                                              _fp(out), out.size, frames.ctypes.data_as(_u32p)))
        return self._collect(out, frames, cap)

    def push_stft(self, ids: Sequence[int], chunks: Sequence, dtype=np.complex128, full: bool = True) -> List[np.ndarray]:
        """push() emitting what Spectrogram::add returns (src/stft.rs:48-86): [k_i, bins] complex spectra per stream."""
        a, _, flat, lens, cap, frames = self._gather(ids, chunks, False)
        dt = np.dtype(dtype)
        out = np.empty((cap, self._mel.stft_bins(full)), dt)
        _check(lib().melspec_stream_push_host_stft(self._h, a.ctypes.data_as(_u32p), _fp(flat), lens.ctypes.data_as(_u32p), a.shape[0],
                                                   out.ctypes.data_as(C.c_void_p), out.size, frames.ctypes.data_as(_u32p),
                                                   int(dt == np.dtype(np.complex128)), int(full)))
        return self._collect(out, frames, cap)

    def flush(self, ids: Sequence[int]) -> List[np.ndarray]:
        """Spectrogram::add with the pending (< hop) samples: zero-padded, at most one more frame per stream."""
        a, out, frames = self._flush_args(ids)
        _check(lib().melspec_stream_flush_host(self._h, a.ctypes.data_as(_u32p), a.shape[0], _fp(out), out.size, frames.ctypes.data_as(_u32p)))
        return self._collect(out, frames)

    # ---- int16 PCM chunks in, f16 / bf16 rows out (melspec_stream_*_io) ----
    def supports_io(self, pcm_dtype: int, out_dtype: int) -> bool:
        return bool(lib().melspec_stream_supports_io(self._h, int(pcm_dtype), int(out_dtype)))

    def push_io(self, ids: Sequence[int], chunks: Sequence, out_dtype=None) -> List[np.ndarray]:
        """push() with typed ends: np.int16 chunks are 16-bit PCM (value = sample / 32768, exactly) and cross the bus as such -- all
        chunks of one call have the same dtype; out_dtype "f16" (or np.float16) returns np.float16 rows, "bf16" the bfloat16 bit
        patterns as np.uint16 (numpy has no bfloat16): the f32 rows of push() rounded to nearest even."""
        a, pcm, flat, lens, cap, frames = self._gather(ids, chunks, True)
        out_code = _out_code(out_dtype)
        out = np.empty((cap, self.n_mels), _OUT_NUMPY[out_code])
        _check(lib().melspec_stream_push_host_io(self._h, a.ctypes.data_as(_u32p), flat.ctypes.data_as(C.c_void_p), pcm,
                                                 lens.ctypes.data_as(_u32p), a.shape[0], out.ctypes.data_as(C.c_void_p), out_code, out.size,
                                                 frames.ctypes.data_as(_u32p)))
        return self._collect(out, frames, cap)

    def flush_io(self, ids: Sequence[int], out_dtype) -> List[np.ndarray]:
        """flush() whose rows have the type of push_io's out_dtype"""
        out_code = _out_code(out_dtype)
        a, out, frames = self._flush_args(ids, _OUT_NUMPY[out_code])
        _check(lib().melspec_stream_flush_host_io(self._h, a.ctypes.data_as(_u32p), a.shape[0], out.ctypes.data_as(C.c_void_p), out_code,
                                                  out.size, frames.ctypes.data_as(_u32p)))
        return self._collect(out, frames)

    # ---- the detector stage: VoiceActivityDetector::add_activity per stream, inside the push (src/vad.rs:155-205) ----
    def enable_vad(self, settings: Optional[DetectionSettings], timing: Optional[VadFrameTiming] = None) -> None:
        """Every push / flush from now on also feeds each stream's detector on the device; None turns the stage off.
        timing (VoiceActivityDetector::new_with_timing, src/vad.rs:149-153): records then carry their timestamps."""
        self._vad_timing = timing
        if settings is None:
            _check(lib().melspec_stream_enable_vad(self._h, None))
        else:
            c = settings._c()
            _check(lib().melspec_stream_enable_vad(self._h, C.byref(c)))

    def vad_frames(self, stream: int) -> int:
        """frames the stream has fed to its detector: VoiceActivityDetector::frame_index of the next one"""
        return int(lib().melspec_stream_vad_frames(self._h, stream))

    def _activities(self, ids: np.ndarray, first: Sequence[int], acts: np.ndarray, frames: np.ndarray) -> List[List[Optional[VoiceActivity]]]:
        res, cur = [], 0
        for i in range(ids.shape[0]):
            rows = []
            for k in range(int(frames[i])):
                a = acts[cur + k]
                if not a["valid"]:
                    rows.append(None)                   # add_activity returned None: fewer than min_x frames so far
                    continue
                w, n = int(a["window_columns"]), int(a["active_columns"])
                t = getattr(self, "_vad_timing", None)
                rows.append(VoiceActivity(bool(a["active"]), first[i] + k, int(a["leading_active_columns"]), n, w, 0.0 if w == 0 else n / w,
                                          None if t is None else t.timestamps_for_frame(first[i] + k)))
            res.append(rows)
            cur += int(frames[i])
        return res

    def push_vad(self, ids: Sequence[int], chunks: Sequence):
        """push() that also returns, per stream, what add_activity gives for each emitted frame (None or VoiceActivity)."""
        a, _, flat, lens, cap, frames = self._gather(ids, chunks, False)
        first = [self.vad_frames(int(s)) for s in a]
        out = np.empty((cap, self.n_mels), np.float32)
        acts = np.zeros(cap, ACTIVITY_DTYPE)
        _check(lib().melspec_stream_push_host_vad(self._h, a.ctypes.data_as(_u32p), _fp(flat), lens.ctypes.data_as(_u32p), a.shape[0],
                                                  _fp(out), out.size, frames.ctypes.data_as(_u32p), acts.ctypes.data_as(C.c_void_p), cap))
        return self._collect(out, frames, cap), self._activities(a, first, acts, frames)

    def flush_vad(self, ids: Sequence[int]):
        a, out, frames = self._flush_args(ids)
        first = [self.vad_frames(int(s)) for s in a]
        acts = np.zeros(a.shape[0], ACTIVITY_DTYPE)
        _check(lib().melspec_stream_flush_host_vad(self._h, a.ctypes.data_as(_u32p), a.shape[0], _fp(out), out.size, frames.ctypes.data_as(_u32p),
                                                   acts.ctypes.data_as(C.c_void_p), acts.shape[0]))
        return self._collect(out, frames), self._activities(a, first, acts, frames)

    # ---- device producers (input_ptr: where a stream's next chunk goes) ---------------------
    def push_device(self, ids: Sequence[int], lens: Sequence[int], d_out: int, out_offsets=None, stream: int = 0) -> np.ndarray:
        frames, n, (p_ids, p_lens, p_oo), _arrs = self._dev(ids, lens, out_offsets)
        _check(lib().melspec_stream_push_device(self._h, p_ids, p_lens, n, C.c_void_p(d_out), p_oo, frames.ctypes.data_as(_u32p), C.c_void_p(stream)))
        return frames

    def push_device_io(self, ids: Sequence[int], d_chunks: int, pcm_dtype: int, lens: Sequence[int], d_out: int, out_dtype: int,
                       src_offsets=None, out_offsets=None, stream: int = 0) -> np.ndarray:
        """push_device with typed ends.  d_chunks != 0: chunk i is lens[i] elements of pcm_dtype (PCM_F32 / PCM_S16) at d_chunks +
        src_offsets[i] elements (None: back to back), anywhere in device memory; d_chunks == 0: the chunks are at input_ptr, in f32.
        Rows of out_dtype (OUT_F32 / OUT_F16 / OUT_BF16) go to d_out + out_offsets[i] elements (None: back to back)."""
        frames, n, (p_ids, p_lens, p_oo, p_so), _arrs = self._dev(ids, lens, out_offsets, src_offsets)
        _check(lib().melspec_stream_push_device_io(self._h, p_ids, C.c_void_p(d_chunks or None), int(pcm_dtype), p_so, p_lens, n, C.c_void_p(d_out or None),
                                                   int(out_dtype), p_oo, frames.ctypes.data_as(_u32p), C.c_void_p(stream or None)))
        return frames

    def push_device_vad(self, ids: Sequence[int], lens: Sequence[int], d_out: int, d_acts: int, out_offsets=None, stream: int = 0) -> np.ndarray:
        """push_device whose activity records (ACTIVITY_DTYPE, packed in entry order) go to device memory at d_acts."""
        frames, n, (p_ids, p_lens, p_oo), _arrs = self._dev(ids, lens, out_offsets)
        _check(lib().melspec_stream_push_device_vad(self._h, p_ids, p_lens, n, C.c_void_p(d_out), p_oo, frames.ctypes.data_as(_u32p), C.c_void_p(d_acts),
                                                    C.c_void_p(stream)))
        return frames


class _StatBank(_Bank):
    """What the Kaldi and the NeMo / Parakeet bank share (csrc/stat_bank.hpp's StatBank): the calls behind their pushes and stats.  A
    subclass states its prefix (_P), keeps its owner alive, and says how the flat output of a host call splits per stream (_cut)."""

    def _open(self, owner_handle, n_streams: int, max_chunk: int, n_mels: int) -> None:
        self.n_streams, self.max_chunk, self.n_mels = int(n_streams), int(max_chunk), int(n_mels)
        h = C.c_void_p()
        _check(self._fn("create")(C.byref(h), owner_handle, self.n_streams, self.max_chunk), construct=True)
        self._h = h

    def _cut(self, out: np.ndarray, frames: np.ndarray) -> List[np.ndarray]:
        raise NotImplementedError

    def _host(self, name: str, a: np.ndarray, cap: int, out_code: Optional[int], *src) -> tuple:
        """the host call `name` (out_code None) or its _io form; src: its arguments between ids and n.  Returns (the output cut per
        stream, the frames each emitted)"""
        out = np.empty(cap * self.n_mels, np.float32 if out_code is None else _OUT_NUMPY[out_code])
        frames = np.zeros(a.shape[0], np.uint32)
        dst = (_fp(out),) if out_code is None else (out.ctypes.data_as(C.c_void_p), out_code)
        _check(self._fn(name if out_code is None else name + "_io")(self._h, a.ctypes.data_as(_u32p), *src, a.shape[0], *dst, out.size, frames.ctypes.data_as(_u32p)))
        return self._cut(out, frames), frames

    def _push(self, ids: Sequence[int], chunks: Sequence, out_code: Optional[int] = None) -> List[np.ndarray]:
        a, pcm, flat, lens, cap, _ = self._gather(ids, chunks, True)
        res, frames = self._host("push_host", a, cap, out_code, flat.ctypes.data_as(C.c_void_p), pcm, lens.ctypes.data_as(_u32p))
        assert int(frames.sum()) == cap
        return res

    def _device(self, name: str, ids, lens, d_out, out_offsets, stream, out_dtype: Optional[int], src=None) -> np.ndarray:
        """the device call `name` (out_dtype None) or its _io form; src: a push's (d_chunks, pcm_dtype, src_offsets), None where the call
        takes no chunks.  Returns the frames each stream emitted"""
        frames, n, (p_ids, p_lens, p_oo, p_so), _arrs = self._dev(ids, lens, out_offsets, src and src[2])
        chunks = () if src is None else (C.c_void_p(src[0] or None), int(src[1]), p_so, p_lens)
        dst = (C.c_void_p(d_out or None),) if out_dtype is None else (C.c_void_p(d_out or None), int(out_dtype))
        _check(self._fn(name if out_dtype is None else name + "_io")(self._h, p_ids, *chunks, n, *dst, p_oo, frames.ctypes.data_as(_u32p), C.c_void_p(stream or None)))
        return frames

    def _push_device(self, ids, lens, d_out, out_offsets, d_chunks, pcm_dtype, src_offsets, stream, out_dtype: Optional[int] = None) -> np.ndarray:
        return self._device("push_device", ids, lens, d_out, out_offsets, stream, out_dtype, (d_chunks, pcm_dtype, src_offsets))

    def supports_io(self, pcm_dtype: int, out_dtype: int) -> bool:
        return bool(self._fn("supports_io")(self._h, int(pcm_dtype), int(out_dtype)))

    def _stats(self, ids: Sequence[int], k: int) -> tuple:
        """stats_host: (k arrays [n, n_mels] f32, counts [n] u64)"""
        a = _u32(ids)
        arrs = [np.zeros((a.shape[0], self.n_mels), np.float32) for _ in range(k)]
        counts = np.zeros(a.shape[0], np.uint64)
        _check(self._fn("stats_host")(self._h, a.ctypes.data_as(_u32p), a.shape[0], *[_fp(x) for x in arrs], counts.ctypes.data_as(C.POINTER(C.c_uint64))))
        return (*arrs, counts)

    def _stats_device(self, ids: Sequence[int], stream: int, *d_arrs: int) -> np.ndarray:
        a = _u32(ids)
        counts = np.zeros(a.shape[0], np.uint64)
        _check(self._fn("stats_device")(self._h, a.ctypes.data_as(_u32p), a.shape[0], *[C.c_void_p(d or None) for d in d_arrs],
                                        counts.ctypes.data_as(C.POINTER(C.c_uint64)), C.c_void_p(stream or None)))
        return counts


class FbankStreamBank(_StatBank):
    """n_streams independent Fbank::compute streams (src/fbank.rs:141-236) on one Fbank's geometry (melspec_fbank_stream_*): after pushes
    whose chunks concatenate to x a stream has emitted exactly the rows of Fbank::compute(x) with apply_cmn off -- the bits of
    Fbank.compute on an apply_cmn = False twin, however x was cut -- and stats() returns the running column means of those rows.
    The Fbank must be on the fused path (uses_fast_path) with frame_shift <= frame_length."""
    _P = "melspec_fbank_stream_"

    def __init__(self, fbank, n_streams: int, max_chunk: int):
        self._fbank = fbank                  # keeps the object alive
        self._open(fbank._h, n_streams, max_chunk, fbank.num_mel_bins)

    def _cut(self, out: np.ndarray, frames: np.ndarray) -> List[np.ndarray]:
        return self._collect(out.reshape(-1, self.n_mels), frames)

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        """no history, no frames, zero sums for the listed streams (None: all)"""
        super().reset(ids)

    def push(self, ids: Sequence[int], chunks: Sequence) -> List[np.ndarray]:
        """Append chunks[i] (any length <= max_chunk; np.int16 chunks are 16-bit PCM, value = sample / 32768 exactly, and all chunks of
        one call have the same dtype) to stream ids[i]; returns the rows each stream emitted, [k_i, num_mel_bins], before CMN."""
        return self._push(ids, chunks)

    def push_device(self, ids: Sequence[int], lens: Sequence[int], d_out: int, out_offsets=None, d_chunks: int = 0, pcm_dtype: int = PCM_F32,
                    src_offsets=None, stream: int = 0) -> np.ndarray:
        """d_chunks == 0: the chunks are at input_ptr, in f32; otherwise chunk i is lens[i] elements of pcm_dtype at d_chunks +
        src_offsets[i] elements (None: back to back).  Rows go to d_out + out_offsets[i] floats (None: back to back)."""
        return self._push_device(ids, lens, d_out, out_offsets, d_chunks, pcm_dtype, src_offsets, stream)

    # ---- f16 / bf16 rows out (melspec_fbank_stream_*_io): the statistics stay those of the f32 rows ----
    def push_io(self, ids: Sequence[int], chunks: Sequence, out_dtype=None) -> List[np.ndarray]:
        """push() whose rows have the type out_dtype names: None np.float32, "f16" (or np.float16) np.float16, "bf16" the bfloat16 bit
        patterns as np.uint16 -- the f32 rows of push() rounded to nearest even.  stats() is what it is after the same push()es."""
        return self._push(ids, chunks, _out_code(out_dtype))

    def supports_io(self, pcm_dtype: int, out_dtype: int) -> bool:
        """every valid pair of codes, on every Fbank a bank can be created on"""
        return super().supports_io(pcm_dtype, out_dtype)

    def push_device_io(self, ids: Sequence[int], d_chunks: int, pcm_dtype: int, lens: Sequence[int], d_out: int, out_dtype: int,
                       src_offsets=None, out_offsets=None, stream: int = 0) -> np.ndarray:
        """push_device with typed rows: d_chunks / pcm_dtype / src_offsets as there; rows of out_dtype (OUT_F32 / OUT_F16 / OUT_BF16) go to
        d_out + out_offsets[i] elements (None: back to back; a 16-bit entry may start at an odd element)."""
        return self._push_device(ids, lens, d_out, out_offsets, d_chunks, pcm_dtype, src_offsets, stream, out_dtype)

    def stats(self, ids: Sequence[int]):
        """(means [n, num_mel_bins] f32, counts [n] u64): mean[bin] = f32(f64 sum of the stream's emitted rows / their count), zeros for
        a stream without a row"""
        return self._stats(ids, 1)

    def stats_device(self, ids: Sequence[int], d_means: int, stream: int = 0) -> np.ndarray:
        """the means to device memory at d_means ([n, num_mel_bins] f32); returns the counts"""
        return self._stats_device(ids, stream, d_means)


class BlmStreamBank(_StatBank):
    """n_streams independent BatchLogMelSpectrogram::compute streams (src/mel.rs) on one BatchLogMelSpectrogram's geometry
    (melspec_blm_stream_*): after pushes whose chunks concatenate to x and one finish, a stream has emitted exactly the columns of
    compute(x) on a normalize_per_feature = False twin in the same precision mode (pad_to ignored) -- bit for bit, however x was cut
    -- and stats() returns the running per-feature mean and 1 / (std + 1e-5) of those columns (Welford in f64, in time order).
    The frontend must be on the fused kernels (n_fft = 512, win_length = 400)."""
    _P = "melspec_blm_stream_"

    def __init__(self, blm, n_streams: int, max_chunk: int):
        self._blm = blm                      # keeps the context alive
        self._open(blm._h, n_streams, max_chunk, blm.config.n_mels)

    def _cut(self, out: np.ndarray, frames: np.ndarray) -> List[np.ndarray]:
        res, cur = [], 0
        for f in frames:
            n = int(f) * self.n_mels
            res.append(out[cur:cur + n].reshape(self.n_mels, int(f)))
            cur += n
        return res

    def reset(self, ids: Optional[Sequence[int]] = None) -> None:
        """no history, no frames, not ended, zero statistics for the listed streams (None: all)"""
        super().reset(ids)

    def finish_frames(self, stream: int) -> int:
        return int(self._fn("finish_frames")(self._h, stream))

    def _finish(self, ids: Sequence[int], out_code: Optional[int] = None) -> List[np.ndarray]:
        a = _u32(ids)
        return self._host("finish_host", a, sum(self.finish_frames(int(s)) for s in a), out_code)[0]

    def _finish_device(self, ids, d_out, out_offsets, stream, out_dtype: Optional[int] = None) -> np.ndarray:
        return self._device("finish_device", ids, [0] * len(ids), d_out, out_offsets, stream, out_dtype)

    def push(self, ids: Sequence[int], chunks: Sequence) -> List[np.ndarray]:
        """Append chunks[i] (any length <= max_chunk; np.int16 chunks are 16-bit PCM, value = sample / 32768 exactly, and all chunks of
        one call have the same dtype) to stream ids[i]; returns the un-normalised columns each stream emitted, [n_mels, k_i]."""
        return self._push(ids, chunks)

    def finish(self, ids: Sequence[int]) -> List[np.ndarray]:
        """End the listed streams: the columns that read past the stream's end (zero padding), [n_mels, k_i]; nothing for an empty stream."""
        return self._finish(ids)

    def push_device(self, ids: Sequence[int], lens: Sequence[int], d_out: int, out_offsets=None, d_chunks: int = 0, pcm_dtype: int = PCM_F32,
                    src_offsets=None, stream: int = 0) -> np.ndarray:
        """d_chunks == 0: the chunks are at input_ptr, in f32; otherwise chunk i is lens[i] elements of pcm_dtype at d_chunks +
        src_offsets[i] elements (None: back to back).  Entry i's [n_mels, k_i] rows go to d_out + out_offsets[i] floats (None: back to back)."""
        return self._push_device(ids, lens, d_out, out_offsets, d_chunks, pcm_dtype, src_offsets, stream)

    def finish_device(self, ids: Sequence[int], d_out: int, out_offsets=None, stream: int = 0) -> np.ndarray:
        return self._finish_device(ids, d_out, out_offsets, stream)

    # ---- f16 / bf16 rows out (melspec_blm_stream_*_io): the statistics stay those of the f32 rows ----
    def push_io(self, ids: Sequence[int], chunks: Sequence, out_dtype=None) -> List[np.ndarray]:
        """push() whose columns have the type out_dtype names: None np.float32, "f16" (or np.float16) np.float16, "bf16" the bfloat16 bit
        patterns as np.uint16 -- the f32 columns of push() rounded to nearest even.  stats() is what it is after the same push()es."""
        return self._push(ids, chunks, _out_code(out_dtype))

    def finish_io(self, ids: Sequence[int], out_dtype=None) -> List[np.ndarray]:
        """finish() whose columns have the type of push_io's out_dtype"""
        return self._finish(ids, _out_code(out_dtype))

    def supports_io(self, pcm_dtype: int, out_dtype: int) -> bool:
        """every valid pair of codes, on every frontend a bank can be created on"""
        return super().supports_io(pcm_dtype, out_dtype)

    def push_device_io(self, ids: Sequence[int], d_chunks: int, pcm_dtype: int, lens: Sequence[int], d_out: int, out_dtype: int,
                       src_offsets=None, out_offsets=None, stream: int = 0) -> np.ndarray:
        """push_device with typed rows: d_chunks / pcm_dtype / src_offsets as there; entry i's [n_mels, k_i] rows of out_dtype (OUT_F32 /
        OUT_F16 / OUT_BF16) go to d_out + out_offsets[i] elements (None: back to back; a 16-bit entry may start at an odd element)."""
        return self._push_device(ids, lens, d_out, out_offsets, d_chunks, pcm_dtype, src_offsets, stream, out_dtype)

    def finish_device_io(self, ids: Sequence[int], d_out: int, out_dtype: int, out_offsets=None, stream: int = 0) -> np.ndarray:
        """finish_device whose columns of out_dtype (OUT_F32 / OUT_F16 / OUT_BF16) go to d_out + out_offsets[i] elements (None: back to back)"""
        return self._finish_device(ids, d_out, out_offsets, stream, out_dtype)

    def stats(self, ids: Sequence[int]):
        """(mean [n, n_mels] f32, inv_std [n, n_mels] f32, counts [n] u64) of the columns the streams have emitted so far: inv_std =
        1 / (sqrt(M2 / max(count - 1, 1)) + 1e-5); mean 0 and inv_std 1e5 for a stream without a column"""
        return self._stats(ids, 2)

    def stats_device(self, ids: Sequence[int], d_mean: int, d_inv_std: int, stream: int = 0) -> np.ndarray:
        """mean and inv_std to device memory ([n, n_mels] f32 each); returns the counts"""
        return self._stats_device(ids, stream, d_mean, d_inv_std)


class RingBuffer:
    """One stream with the reference's interface (src/rb.rs:18-121): add_frame / add feed samples, maybe_mel
    returns one (n_mels, 1) column per completed hop or None.  Frames are computed on the device in batches
    whenever maybe_mel runs dry, so calling it in the reference's `while let Some(mel) = rb.maybe_mel()` loop
    costs one launch per add_frame, not one per hop."""

    def __init__(self, mel: HipMelSpectrogram, capacity: int = 16384):
        self._bank = StreamBank(mel, 1, max(int(capacity), mel.hop_size))
        self._buf = deque()
        self._n = 0
        self._capacity = max(int(capacity), mel.hop_size)
        self._ready = deque()

    def add_frame(self, samples) -> None:
        x = _f32(samples).ravel()
        # src/rb.rs:60-68: when full, the oldest samples are dropped
        over = self._n + x.shape[0] - self._capacity
        while over > 0 and self._buf:
            head = self._buf[0]
            if head.shape[0] <= over:
                self._buf.popleft(); self._n -= head.shape[0]; over -= head.shape[0]
            else:
                self._buf[0] = head[over:]; self._n -= over; over = 0
        if x.shape[0] > self._capacity:
            x = x[-self._capacity:]
        self._buf.append(x)
        self._n += x.shape[0]

    def add(self, sample: float) -> None:
        self.add_frame(np.array([sample], np.float32))

    def maybe_mel(self) -> Optional[np.ndarray]:
        if not self._ready and self._n:
            x = np.concatenate(list(self._buf))
            self._buf.clear(); self._n = 0
            for f in self._bank.push([0], [x])[0]:
                self._ready.append(f)
        if not self._ready:
            return None
        return self._ready.popleft().astype(np.float64).reshape(-1, 1)

    def close(self) -> None:
        self._bank.close()


class Spectrogram:
    """Spectrogram::{new, add} (src/stft.rs:25-86) with the overlap-save state on the device: add(frames) takes at most hop_size
    samples and returns the [fft_size] complex128 spectrum of the window that ends with them once fft_size samples have been seen,
    else None.  A block shorter than hop_size is zero-padded like the reference's (:57-60); the reference then advances its sample
    count by the real samples only, this mirror by a whole hop -- which matters only for when the very first frame of a stream
    appears.  compute_all_cpu is HipMelSpectrogram.compute_all."""

    def __init__(self, fft_size: int, hop_size: int, device: int = -1):
        self.fft_size, self.hop_size = int(fft_size), int(hop_size)
        self._mel = HipMelSpectrogram(self.fft_size, self.hop_size, 16000.0, 1, device=device)     # geometry only: no mel stage is run
        self._bank = StreamBank(self._mel, 1, self.hop_size)

    def add(self, frames) -> Optional[np.ndarray]:
        x = _f32(frames).ravel()
        assert x.shape[0] <= self.hop_size, "frames must be <= hop_size"
        if x.shape[0] < self.hop_size:
            x = np.concatenate([x, np.zeros(self.hop_size - x.shape[0], np.float32)])
        out = self._bank.push_stft([0], [x], np.complex128, True)[0]
        return out[0] if out.shape[0] else None

    def close(self) -> None:
        self._bank.close(); self._mel.close()


class MelSpectrogram:
    """MelSpectrogram::{new, add} (src/mel.rs:13-32): add(fft) projects one spectrum ([fft_size] complex, what Spectrogram::add
    returns) onto the Slaney bank, log10, per-frame normalisation -> (n_mels, 1) float64 like the reference's Array2<f64>."""

    def __init__(self, fft_size: int, sampling_rate: float, n_mels: int, device: int = -1):
        from .hip import SparseMelFilterbank
        self._bank = SparseMelFilterbank.from_mel(float(sampling_rate), int(fft_size), int(n_mels), device=device)

    def add(self, fft) -> np.ndarray:
        # full f64 like the reference (project_stft_log10 src/mel.rs:148-168, then norm_mel over the frame :645-654): the device's
        # log_mel_spectrogram + norm_mel in f64 (round 4; the mel_from_stft route returned f32 values widened)
        a = np.ascontiguousarray(fft, np.complex128).reshape(1, -1)
        return self._bank.norm_mel(self._bank.log_mel_spectrogram(a)[0]).reshape(-1, 1)

    def close(self) -> None:
        self._bank.close()

