"""mel_spec_amd -- MI355X (gfx950) log-mel spectrogram frontend behind the API of
wavey-ai/mel-spec's GPU plugin slot.  All compute runs in hand-written HIP kernels
(csrc/) reached through the C ABI of libmelspec_hip.so (include/melspec_hip.h)."""
from .hip import (BatchLogMelConfig, BatchLogMelError, BatchLogMelSpectrogram, DeviceBuffer, HostBuffer, Fbank, FbankConfig, HipError, HipMelSpectrogram, HipRuntimeError, HipUnavailable, SparseMelFilterbank,
                  blm_compute_ragged_device_desc, blm_compute_ragged_device_split, blm_compute_ragged_device_split_io, blm_compute_ragged_split, blm_compute_ragged_split_io,
                  blm_compute_split_io, blm_compute_uniform_device_split_io, blm_supports_split_io, fbank_compute_ragged_device_split, fbank_compute_ragged_device_split_io,
                  fbank_compute_ragged_split_io, fbank_compute_split_io, fbank_compute_uniform_device_split_io, fbank_supports_split_io, supports_whisper, whisper_kernel_name, whisper_num_frames, whisper_uniform_device, whisper_ragged_device, whisper_uniform_device_split, whisper_ragged_device_split, whisper_features, whisper_features_batch, whisper_split, device_count, device_synchronize, fft_frequencies, hann_window, hz_to_mel, kaldi_mel_filterbank, mel, mel_frequencies, mel_to_hz,
                  mels_to_hz, synth_pcm_device, synth_pcm_window)
from .parallel import ShardedMelSpectrogram, gather_peer, shard_by_samples, shard_range
from .quant import QuantizationRange, TgaCodec, chunk_frames_into_strides, to_array2
from .stream import BlmStreamBank, FbankStreamBank, MelSpectrogram, RingBuffer, Spectrogram, StreamBank
from .vad import (DetectionSettings, EdgeInfo, VadFrameTiming, VoiceActivity, VoiceActivityDetector, VoiceActivityTimestamps, duration_ms_for_n_frames,
                  format_milliseconds, n_frames_for_duration, vad_boundaries, vad_boundaries_device, vad_mask_len, vad_on)

__all__ = ["BatchLogMelConfig", "BatchLogMelError", "BatchLogMelSpectrogram", "DeviceBuffer", "HostBuffer", "Fbank", "FbankConfig", "HipError", "HipMelSpectrogram", "HipRuntimeError", "SparseMelFilterbank",
           "HipUnavailable", "blm_compute_ragged_device_desc", "blm_compute_ragged_device_split", "blm_compute_ragged_split", "blm_supports_split_io", "blm_compute_uniform_device_split_io",
           "blm_compute_split_io", "blm_compute_ragged_device_split_io", "blm_compute_ragged_split_io", "fbank_supports_split_io", "fbank_compute_ragged_device_split", "supports_whisper", "whisper_kernel_name", "whisper_num_frames", "whisper_uniform_device", "whisper_ragged_device", "whisper_uniform_device_split", "whisper_ragged_device_split", "whisper_features", "whisper_features_batch", "whisper_split",
           "fbank_compute_uniform_device_split_io", "fbank_compute_ragged_device_split_io", "fbank_compute_split_io", "fbank_compute_ragged_split_io", "device_count", "device_synchronize", "hann_window", "kaldi_mel_filterbank", "mel", "hz_to_mel", "mel_to_hz", "mels_to_hz", "mel_frequencies", "fft_frequencies",
           "synth_pcm_device", "synth_pcm_window", "shard_range", "shard_by_samples", "ShardedMelSpectrogram", "gather_peer", "QuantizationRange", "TgaCodec", "to_array2", "chunk_frames_into_strides", "RingBuffer", "StreamBank", "FbankStreamBank", "BlmStreamBank", "Spectrogram", "MelSpectrogram", "DetectionSettings", "EdgeInfo", "VoiceActivity", "VoiceActivityDetector", "VadFrameTiming", "VoiceActivityTimestamps", "n_frames_for_duration", "duration_ms_for_n_frames", "format_milliseconds",
           "vad_boundaries", "vad_boundaries_device", "vad_mask_len", "vad_on"]
