"""The public Python surface of the three frontends (mel_spec_amd/hip.py), pinned name by name: every public attribute of
HipMelSpectrogram, Fbank and BatchLogMelSpectrogram with str(inspect.signature(...)) for a method, "property" for a property and the repr
for anything else.  The table was written from the classes as they stood before they got their shared base (_Frontend); bench.py, tools/
and parallel.py call these names with these arguments.  The one addition since: BatchLogMelSpectrogram.compute_ragged_device, which the
class's compute_ragged used to spell out as a raw ctypes call."""
import inspect

import pytest

UNIFORM = "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_out: 'int', stream: 'int' = 0) -> 'None'"
UNIFORM_IO = "(self, d_pcm: 'int', pcm_dtype: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_out: 'int', out_dtype: 'int', stream: 'int' = 0) -> 'None'"
RAGGED = "(self, d_pcm: 'int', offsets, lengths, d_out: 'int', out_offsets=None, stream: 'int' = 0) -> 'None'"
RAGGED_IO = "(self, d_pcm: 'int', pcm_dtype: 'int', offsets, lengths, d_out: 'int', out_dtype: 'int', out_offsets=None, stream: 'int' = 0) -> 'None'"
RAGGED_DESC = "(self, d_pcm: 'int', d_offsets: 'int', d_lengths: 'int', n_clips: 'int', d_out: 'int', d_out_offsets: 'int', max_total_frames: 'int', stream: 'int' = 0) -> 'None'"
BATCH_HOST = "(self, flat: 'np.ndarray', offsets, lengths, out: 'np.ndarray | None' = None, out_offsets=None)"
SUPPORTS_IO = "(self, pcm_dtype: 'int', out_dtype: 'int') -> 'bool'"
NUM_FRAMES = "(self, n_samples: 'int') -> 'int'"
SYNCHRONIZE = "(self, stream: 'int' = 0) -> 'None'"
NONE = "(self) -> 'None'"
CLIPS_LIST = "(self, clips) -> 'list'"
CLIPS_ARRAY = "(self, clips) -> 'np.ndarray'"
SAMPLES_ARRAY = "(self, samples) -> 'np.ndarray'"
HOST_IO = "(self, samples, out_dtype=None) -> 'np.ndarray'"

SURFACE = {
    "HipMelSpectrogram": {
        "PRECISION": "{'auto': 0, 'f64': 1, 'f32': 2}",
        "auto_state": "(self)",
        "close": NONE,
        "compute_all": "(self, samples, dtype=<class 'numpy.complex128'>, full: 'bool' = True) -> 'np.ndarray'",
        "compute_batch": CLIPS_ARRAY,
        "compute_batch_host": BATCH_HOST,
        "compute_batch_interleaved": "(self, clips, major_column_order: 'bool' = False, min_width: 'int' = 0) -> 'np.ndarray'",
        "compute_mel_spectrogram": HOST_IO,
        "compute_ragged": CLIPS_LIST,
        "compute_ragged_device": RAGGED,
        "compute_ragged_device_desc": RAGGED_DESC,
        "compute_ragged_device_io": RAGGED_IO,
        "compute_uniform_device": UNIFORM,
        "compute_uniform_device_interleaved": "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_out: 'int', "
                                              "major_column_order: 'bool' = False, min_width: 'int' = 0, stream: 'int' = 0) -> 'None'",
        "compute_uniform_device_io": UNIFORM_IO,
        "guard_count": "(self) -> 'int'",
        "guard_last_count": "(self) -> 'int'",
        "interleaved_width": "(self, n_samples: 'int', min_width: 'int' = 0) -> 'int'",
        "mel_from_stft": "(self, spec) -> 'np.ndarray'",
        "mel_from_stft_device": "(self, d_spec: 'int', n_frames: 'int', d_out: 'int', f64: 'bool' = False, full: 'bool' = False, stream: 'int' = 0) -> 'None'",
        "num_frames": NUM_FRAMES,
        "plain_kernel_name": "(self) -> 'str'",
        "precise": "property",
        "precision": "property",
        "release_scratch": NONE,
        "set_auto_adaptive": "(self, on: 'bool' = True) -> 'None'",
        "set_precise": "(self, on: 'bool' = True) -> 'None'",
        "set_precision": "(self, mode: 'str') -> 'None'",
        "stft_bins": "(self, full: 'bool' = False) -> 'int'",
        "stft_ragged_device": "(self, d_pcm: 'int', offsets, lengths, d_out: 'int', out_offsets=None, f64: 'bool' = False, full: 'bool' = False, stream: 'int' = 0) -> 'None'",
        "stft_uniform_device": "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_out: 'int', f64: 'bool' = False, "
                               "full: 'bool' = False, stream: 'int' = 0) -> 'None'",
        "supports_io": SUPPORTS_IO,
        "synchronize": SYNCHRONIZE,
        "time_first_kernel": "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_out: 'int', warmup: 'int' = 10, iters: 'int' = 100) -> 'float'",
        "time_uniform_device": "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_out: 'int', warmup: 'int' = 3, iters: 'int' = 20) -> 'float'",
        "uses_fast_path": "property",
    },
    "Fbank": {
        "close": NONE,
        "compute": SAMPLES_ARRAY,
        "compute_batch": CLIPS_ARRAY,
        "compute_batch_host": BATCH_HOST,
        "compute_host_io": HOST_IO,
        "compute_many": CLIPS_LIST,
        "compute_ragged": CLIPS_LIST,
        "compute_ragged_device": RAGGED,
        "compute_ragged_device_desc": RAGGED_DESC,
        "compute_ragged_device_io": RAGGED_IO,
        "compute_uniform_device": UNIFORM,
        "compute_uniform_device_io": UNIFORM_IO,
        "compute_uniform_device_split": "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_rows: 'int', d_means: 'int', stream: 'int' = 0) -> 'None'",
        "dense_filterbank": "(self) -> 'np.ndarray'",
        "num_frames": NUM_FRAMES,
        "release_scratch": NONE,
        "supports_io": SUPPORTS_IO,
        "synchronize": SYNCHRONIZE,
        "use_generic": "(self, on: 'bool' = True) -> 'None'",
        "uses_fast_path": "property",
    },
    "BatchLogMelSpectrogram": {
        "close": NONE,
        "compute": SAMPLES_ARRAY,
        "compute_batch": CLIPS_ARRAY,
        "compute_batch_host": BATCH_HOST,
        "compute_flat": "(self, samples)",
        "compute_host_io": HOST_IO,
        "compute_many": CLIPS_LIST,
        "compute_ragged": CLIPS_LIST,
        "compute_ragged_device_io": RAGGED_IO,
        "compute_split": "(self, samples)",
        "compute_uniform_device": UNIFORM,
        "compute_uniform_device_io": UNIFORM_IO,
        "compute_uniform_device_split": "(self, d_pcm: 'int', clip_stride: 'int', clip_len: 'int', n_clips: 'int', d_rows: 'int', d_mean: 'int', "
                                        "d_inv_std: 'int', stream: 'int' = 0) -> 'None'",
        "filters": "(self, device: 'int' = -1) -> \"'SparseMelFilterbank'\"",
        "num_frames": NUM_FRAMES,
        "padded_frames": NUM_FRAMES,
        "precision": "property",
        "release_scratch": NONE,
        "set_precision": "(self, mode: 'str') -> 'None'",
        "supports_io": SUPPORTS_IO,
        "supports_split": "(self) -> 'bool'",
        "synchronize": SYNCHRONIZE,
    },
}
ADDED = {"BatchLogMelSpectrogram": {"compute_ragged_device": RAGGED}}


def surface(cls):
    out = {}
    for name in dir(cls):
        if name.startswith("_"):
            continue
        a = inspect.getattr_static(cls, name)
        out[name] = "property" if isinstance(a, property) else str(inspect.signature(getattr(cls, name))) if callable(a) else repr(a)
    return out


@pytest.mark.parametrize("name", sorted(SURFACE))
def test_public_surface_is_pinned(name):
    from mel_spec_amd import hip
    assert surface(getattr(hip, name)) == {**SURFACE[name], **ADDED.get(name, {})}
