/*
 * melspec_hip.h -- C ABI of libmelspec_hip.so, the MI355X (gfx950) log-mel frontend.
 *
 * This is the drop-in boundary for the reference's GPU plugin slot.  Each entry point
 * names the reference interface it replaces (paths relative to wavey-ai/mel-spec v0.4.0).
 * The reference binds its CUDA plugin per *stage* (cufftExecZ2Z + launch_mel_kernel,
 * src/cuda.rs:185-219, src/cuda_kernels.cu:49-66); this library is bound per *batch*:
 * one call = framing + Hann + FFT + power + mel + log10 + per-frame normalisation.
 *
 * Conventions (mirroring src/cuda.rs:10-25,164 and src/cuda_kernels.cu:56-58):
 *   - every function returns int; 0 == success (CUDA_SUCCESS analogue);
 *     > 0  == a hipError_t raised by the runtime (maps to CudaError::Runtime);
 *     < 0  == a library code below (INVALID_ARG / UNAVAILABLE map to
 *             CudaError::Unavailable when raised by *_create, Runtime otherwise);
 *   - nothing throws or aborts across the ABI;
 *   - plain pointers and sizes only; the caller owns every buffer it passes in;
 *     the context owns its device tables, scratch, pinned staging and stream;
 *   - a context is single-threaded (one per host thread per device), like
 *     `&mut self` + raw device pointers in CudaMelSpectrogram (src/cuda.rs:27-36);
 *   - *_host calls are synchronous; *_device calls are stream-ordered and asynchronous.
 */
#ifndef MELSPEC_HIP_H
#define MELSPEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MELSPEC_OK                 0
#define MELSPEC_ERR_INVALID_ARG   (-1)  /* zero/oversized sizes, NULL pointers (src/cuda.rs:45-49) */
#define MELSPEC_ERR_UNAVAILABLE   (-2)  /* no HIP device / not gfx950 / runtime missing (tests self-skip, src/cuda.rs:512-518) */
#define MELSPEC_ERR_CAPACITY      (-3)  /* caller's output buffer is too small */
#define MELSPEC_ERR_UNSUPPORTED   (-4)  /* geometry outside what the kernels cover */
#define MELSPEC_ERR_INTERNAL      (-5)

typedef struct melspec_ctx melspec_ctx;      /* Whisper-style log-mel (HipMelSpectrogram) */
typedef struct melspec_sharded melspec_sharded;   /* one melspec_ctx per GPU of the node, clips split per device */
typedef struct melspec_fbank melspec_fbank;  /* Kaldi-style fbank (Fbank)                  */

/* ---- library / device ------------------------------------------------------------- */

/* ABI version of this header (bumped on incompatible change). */
int melspec_abi_version(void);
/* Hash of the sources this library was built from (mel_spec_amd/build.py: the .hip / .hpp files of csrc/ and the headers of include/), "unknown" for a
 * build made by hand.  The test harness rebuilds when it differs from the hash of the checkout, so a stale prebuilt library cannot pass. */
const char *melspec_source_hash(void);
/* Number of usable gfx950 devices, or MELSPEC_ERR_UNAVAILABLE. */
int melspec_device_count(void);
/* Message for the last failure on this thread (valid until the next failing call).
 * Counterpart of the String inside CudaError::Runtime (src/cuda.rs:10-25). */
const char *melspec_last_error(void);

/* ---- Whisper log-mel: replaces CudaMelSpectrogram (src/cuda.rs:27-140) ------------- */

/* CudaMelSpectrogram::new(fft_size, hop_size, sampling_rate, n_mels) (src/cuda.rs:39-82).
 * Builds the periodic Hann window (src/stft.rs:141-145), the Slaney filterbank
 * mel(sr, fft, n_mels, None, None, false, true) (src/mel.rs:19-24,547-589) and FFT
 * twiddles in f64 on the host, uploads them as f32 tables.  device < 0 -> current device. */
int melspec_create(melspec_ctx **out, int device, int fft_size, int hop_size,
                   double sampling_rate, int n_mels);
/* MelSpectrogram with a caller-chosen filterbank instead of new()'s mel(sr, fft, n_mels, None, None, false, true) (src/mel.rs:19-24):
 * SparseMelFilterbank::from_mel(sr, n_fft, n_mels, f_min, f_max, htk, norm) (src/mel.rs:73-87; f_min < 0 == None, f_max <= 0 == None)
 * or from_dense(filters) (src/mel.rs:48-71; row-major [n_mels][fft_size / 2 + 1] f64) -- what log_mel_spectrogram(stft, mel_filters)
 * (src/mel.rs:436-441) takes.  Everything else as melspec_create; a two-filters-per-bin bank (every triangular one) of <= 131 rows
 * runs on the fused n_fft = 400 / 512 kernels, any other matrix on the generic kernel. */
int melspec_create_with_filterbank(melspec_ctx **out, int device, int fft_size, int hop_size, double sampling_rate, int n_mels,
                                   double f_min, double f_max, int htk, int norm);
int melspec_create_with_dense_filterbank(melspec_ctx **out, int device, int fft_size, int hop_size, double sampling_rate, int n_mels,
                                         const double *filters, int fft_bins);
void melspec_destroy(melspec_ctx *ctx);   /* Drop (src/cuda.rs:142-148,366-375) */

/* frame_windows' count: len < fft ? 0 : (len - fft)/hop + 1 (src/stft.rs:153-157). */
size_t melspec_num_frames(const melspec_ctx *ctx, size_t n_samples);
/* CudaMelSpectrogram::max_frames_per_batch (src/cuda.rs:84-86, 150-155: the reference chunks at 8192 frames / 64 MiB): frames
 * per chunk of the host pipeline here (16 MiB of PCM: 26 212 at 400/160).  The device entry points take any batch in one launch. */
size_t melspec_max_frames_per_batch(const melspec_ctx *ctx);
int melspec_fft_size(const melspec_ctx *ctx);
int melspec_hop_size(const melspec_ctx *ctx);
int melspec_n_mels(const melspec_ctx *ctx);
/* 1 if this geometry runs on the fused FFT kernel, 0 if on the generic DFT kernel. */
int melspec_uses_fast_path(const melspec_ctx *ctx);

/* Arithmetic of the fused n_fft = 400 kernels (the reference computes in f64, src/stft.rs:98-111, and its CUDA plugin runs
 * an f64 FFT too, cufftExecZ2Z src/cuda.rs:204-219).  Every mode but F32 is within 1e-4 of the f64 reference on every input.
 *   AUTO (default)  f32 FFT; in the same pass every frame is checked against an empirical error bound -- a mel band within two
 *                   decades of the per-frame clamp (max - 8, src/mel.rs:645-654) is where the f32 FFT's rounding noise can
 *                   exceed 1e-4 (calibrated with tools/flag_calib.py / flag_calib2.py, soaked by tools/fuzz_gpu.py) -- and a
 *                   frame that fails it is recomputed in f64 by the wavefront that owns it (same launch).  Noise-like input
 *                   never takes that branch (the bench workload runs at the f32 rate).  Speech and tonal material trip the
 *                   guard on 40-100 % of their frames, which is slower than computing everything in f64 -- so the launch takes a
 *                   vote first: the first work unit of every wavefront is the sample, and when more than 1/8 of the sampled
 *                   frames trip the guard the f32 kernel stands down and the f64 kernel queued behind it (a second launch that
 *                   returns at once otherwise) computes the whole batch at the F64 rate.  Plain [clip][frame][mel] batches,
 *                   uniform and ragged, and the padded / mel-major layouts (their sample is the head of the batch); only
 *                   melspec_tga_encode_pcm_uniform_device keeps the f32 kernel + recompute whatever the input.  The vote happens inside
 *                   the batch's own launch and nobody waits for it: the result of a call is a function of its input alone (same
 *                   batch -> same bits, whatever the context computed before; round 3 chose from the previous batch's
 *                   statistics).  A clip's bits can differ between two different batches (f32 regime in one, f64 in the other,
 *                   both within 1e-4); F32 and F64 do not have that, nor AUTO after melspec_set_auto_adaptive(ctx, 0).
 *   F64             window, FFT and |X|^2 in f64 for every frame: ~4e-7 from the reference, about 60 % of the f32 rate.
 *   F32             the f32 kernel alone: ~3e-5 on speech and noise, up to ~5e-4 on a line over a floor 70..90 dB down.
 * Geometries on the generic kernels always compute in f64.  The fused n_fft = 512 kernels (Whisper flavour; the 80- and 128-mel banks at
 * 16 kHz have an f32 instantiation) follow the same three modes since round 6:
 *   AUTO  plain [clip][frame][mel] batches, uniform and ragged, of at least two work units per f32 wave of the grid (6144 units = 24 576
 *         frames on an MI355X) run the f32 kernel with the same guard and the same vote; the f64 kernel queued behind it computes the
 *         whole batch on "heavy" and the units the f32 launch noted on "light" (this family has no in-kernel recompute).  Smaller
 *         batches, the padded / mel-major layouts, other banks, and AUTO after melspec_set_auto_adaptive(ctx, 0): the f64 kernel.
 *   F64   the f64 kernel.
 *   F32   the f32 kernel alone, no guard: 2e-5 on speech, ~1e-6 on noise, up to 4e-4 on a line over a floor 70..90 dB down
 *         (profiles/r06_guard512.txt; round 5's f32 instantiation split straight to powers and was 7e-2 off on speech: it now splits to
 *         amplitudes like the n_fft = 400 kernels).
 * melspec_precision() reports the mode in effect (AUTO only where sizeable plain batches do vote, else F64 / F32). */
#define MELSPEC_PRECISION_AUTO 0
#define MELSPEC_PRECISION_F64  1
#define MELSPEC_PRECISION_F32  2
int melspec_set_precision(melspec_ctx *ctx, int mode);
int melspec_precision(const melspec_ctx *ctx);
/* melspec_set_precision(ctx, on ? F64 : AUTO); is_precise: 1 when every frame is computed in f64. */
int melspec_set_precise(melspec_ctx *ctx, int on);
int melspec_is_precise(const melspec_ctx *ctx);
/* Name of the kernel(s) a plain [clip][frame][mel] batch of this context runs on (for profiles and bench lines). */
const char *melspec_plain_kernel_name(const melspec_ctx *ctx);
/* Frames that tripped AUTO's guard since the context was created (f32 kernel: recomputed in f64; f64 kernel: counted only).
 * Synchronises the device. */
int melspec_guard_count(melspec_ctx *ctx, uint64_t *frames);
/* AUTO's vote (default on; 0: the f32 kernel + per-frame recompute whatever the input).  melspec_auto_state reports, without
 * synchronising: *heavy = 1 when the last FINISHED AUTO batch ran on the f64 kernel, *fraction = the fraction of its frames that tripped
 * the guard (batches of >= 256 frames).  Reporting only: nothing is decided from it. */
int melspec_set_auto_adaptive(melspec_ctx *ctx, int on);
int melspec_auto_state(melspec_ctx *ctx, int *heavy, double *fraction);

/* compute_mel_spectrogram(&mut self, samples: &[f32]) -> Vec<Vec<f32>> (src/cuda.rs:88-101)
 * == Spectrogram::compute_mel_spectrogram_cpu (src/stft.rs:119-138) on the GPU.
 * Host PCM in, host [frames][n_mels] f32 out (row-major, src/stft.rs:133-134).
 * Empty/short input -> *n_frames = 0, MELSPEC_OK (src/cuda.rs:91-93). Synchronous. */
int melspec_compute_host(melspec_ctx *ctx, const float *samples, size_t n_samples,
                         float *out, size_t out_capacity_floats, size_t *n_frames);

/* Additive surface: many host clips in one call.  Clip i = samples + offsets[i] (lengths[i] samples); its frames go to
 * out + out_offsets[i] floats (NULL: packed back to back in clip order); *total_frames = frames of all clips.
 * The call is cut into ~16 MiB chunks whose upload, kernels and download overlap on three streams (the reference plugin
 * chunks at 8192 frames with a synchronise per chunk, src/cuda.rs:150-155,343-351); memory from melspec_host_alloc (or
 * any pinned memory) is DMA'd in place, pageable memory is staged through pinned buffers by helper threads.
 * melspec_compute_host takes the same pipeline for clips longer than ~8 MB.  Synchronous. */
int melspec_compute_batch_host(melspec_ctx *ctx, const float *samples, const uint64_t *offsets, const uint64_t *lengths,
                               uint32_t n_clips, float *out, const uint64_t *out_offsets, size_t out_capacity_floats,
                               uint64_t *total_frames);
/* ---- STFT export: Spectrogram::compute_all_cpu (src/stft.rs:89-115) ---------------------------------------------------
 * The complex spectrum of every frame instead of its mel row (callers such as examples/vad_ten_eval/src/main.rs:232-256 feed
 * it to dense mel code of their own).  Always computed in f64 like the reference (frame_windows + forward FFT); stored as
 * interleaved (re, im) pairs of float (MELSPEC_STFT_F32) or double (MELSPEC_STFT_F64), `bins` per frame:
 * full == 0: n_fft/2 + 1 (the input is real); full != 0: n_fft, the reference's Vec<Complex<f64>> layout, upper half =
 * conjugate mirror.  d_out = [clip][frame][bins]; out offsets / capacities count complex elements. */
#define MELSPEC_STFT_F32 0
#define MELSPEC_STFT_F64 1
size_t melspec_stft_bins(const melspec_ctx *ctx, int full);
int melspec_stft_uniform_device(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                void *d_out, int dtype, int full, void *stream);
int melspec_stft_ragged_device(melspec_ctx *ctx, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                               uint32_t n_clips, void *d_out, const uint64_t *h_out_offsets, int dtype, int full, void *stream);
/* compute_all_cpu(samples) on the GPU: host PCM in, host [frames][bins] complex out.  Synchronous. */
int melspec_stft_host(melspec_ctx *ctx, const float *samples, size_t n_samples, void *out, size_t out_capacity_complex,
                      int dtype, int full, size_t *n_frames);

/* ---- the mel stage on its own: MelSpectrogram::add(&fft) (src/mel.rs:13-32) ---------------------------------------------
 * For callers that hold complex STFT frames -- melspec_stft_*'s, or their own (the reference's split API: Spectrogram::add then
 * MelSpectrogram::add): per frame project_stft_log10 (src/mel.rs:148-168: |X[bin]|^2 through the sparse Slaney bank, bins >= n_fft/2
 * contribute nothing, log10(max(E, 1e-10))) and norm_mel_slice_f64 (src/mel.rs:645-654), in f64 like the reference; [frame][n_mels]
 * f32 out.  spec = [frame][bins] interleaved (re, im), dtype / full as in the STFT export (full: n_fft complex per frame, else
 * n_fft/2 + 1). */
int melspec_mel_from_stft_device(melspec_ctx *ctx, const void *d_spec, int dtype, int full, uint64_t n_frames, float *d_out, void *stream);
int melspec_mel_from_stft_host(melspec_ctx *ctx, const void *spec, int dtype, int full, size_t n_frames, float *out, size_t out_capacity_floats);

/* ---- Whisper features as the encoders were trained on them: centred STFT, clip-wide clamp ------------------------------------
 * melspec_compute_* is the reference's streaming-friendly variant (un-centred frames, each clamped against its OWN maximum).
 * openai-whisper's log_mel_spectrogram, Hugging Face's WhisperFeatureExtractor and whisper.cpp compute something else, and these
 * calls compute that.  For a clip x of n samples and the call's pad_to (0: the clip as it is; 480000: Whisper's 30 s; any value
 * >= 400 is legal, 1..399 is MELSPEC_ERR_INVALID_ARG):
 *   1. s = x when pad_to == 0, else x[:pad_to] followed by zeros up to pad_to samples; P = len(s).  P < 400: no frames, and the
 *      clip's maximum (split calls) is -10.
 *   2. T = P / 160 frames (integer division): the centred STFT's last frame is dropped -- 3000 frames for 30 s.
 *   3. frame t = r[160 t .. 160 t + 400) of r = reflect_pad(s, 200) (numpy.pad(mode = "reflect"), torch.stft(center = True)).
 *   4. raw[t][m] = log10(max(E, 1e-10)): periodic Hann, 400-point DFT, |X|^2, the context's Slaney bank -- what the context does.
 *   5. g = the maximum of raw over the WHOLE clip.
 *   6. out[t][m] = (max(raw[t][m], g - 8) + 4) / 4.
 * This is WhisperFeatureExtractor (pad / trim first, then the centred STFT).  openai-whisper pads the waveform by 30 s, transforms and
 * trims the frames afterwards: it differs in frame T - 1 only, and only when n > pad_to - 200 (that frame then sees samples past pad_to
 * instead of their reflection).
 *
 * Contexts: melspec_create(.., 400, 160, 16000.0, 80 | 128) -- the set of melspec_supports_io; every other context gets
 * MELSPEC_ERR_UNSUPPORTED and its output is untouched (melspec_whisper_supports says which).  f32 PCM in, f32 out.
 * Precision (melspec_set_precision): F64 runs the f64 six-frame kernel (80 and 128 mels); F32 the f32 six-frame run kernel at 80 mels and
 * the f64 kernel at 128; AUTO runs the f64 kernel -- the guard, the vote and the in-kernel recompute are calibrated for, and store
 * through, the per-frame clamp, so AUTO's promise (within 1e-4 of the f64 evaluation on every input) is kept by computing in f64 here.
 * The frames that reflect or straddle the end of the samples (a handful per clip) are computed in f64 whatever the mode.
 * melspec_whisper_kernel_name names the kernel of the current mode.
 * int16 PCM in and f16 / bf16 out: the melspec_whisper_*_io calls in the 16-bit section below.
 * A clip table in device memory: the melspec_whisper_compute_ragged_device_desc calls behind the 16-bit section below.
 * NOT covered: a device-resident clip table with pad_to == 0 (the _desc calls need a fixed width); the sharded object; the stream bank.
 *
 * The device calls are stream-ordered and asynchronous (stream NULL: the context's), they do not synchronise with the host and allocate
 * nothing of the caller's; the scratch of the normalised calls (raw rows, one maximum word per clip) is the context's grow-only scratch
 * (melspec_release_scratch gives it back).
 * Normalised output: per clip [T][n_mels] (mel_major == 0) or [n_mels][T] (mel_major != 0: the layout the encoders take) at
 * d_out + h_out_offsets[i] floats (NULL: packed in clip order; uniform: always packed).  With pad_to != 0 every clip has the same T.
 * Split output: d_rows [T][n_mels] per clip = the raw values of step 4 (f32; at d_rows + h_rows_offsets[i], NULL: packed),
 * d_clip_max[n_clips] = g.  Nothing is clamped and no second pass runs: the consumer folds step 6 into its first read. */
int melspec_whisper_supports(const melspec_ctx *ctx);
size_t melspec_whisper_num_frames(const melspec_ctx *ctx, size_t n_samples, size_t pad_to);   /* 0 on a context the calls do not cover */
const char *melspec_whisper_kernel_name(const melspec_ctx *ctx);
int melspec_whisper_compute_uniform_device(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                           uint64_t pad_to, float *d_out, int mel_major, void *stream);
int melspec_whisper_compute_ragged_device(melspec_ctx *ctx, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                          uint32_t n_clips, uint64_t pad_to, float *d_out, const uint64_t *h_out_offsets, int mel_major,
                                          void *stream);
int melspec_whisper_compute_uniform_device_split(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                                 uint32_t n_clips, uint64_t pad_to, float *d_rows, float *d_clip_max, void *stream);
int melspec_whisper_compute_ragged_device_split(melspec_ctx *ctx, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                                uint32_t n_clips, uint64_t pad_to, float *d_rows, const uint64_t *h_rows_offsets,
                                                float *d_clip_max, void *stream);
/* One clip from host memory: upload, the device call, download; synchronous.  out_capacity_floats >= T * n_mels, *n_frames = T. */
int melspec_whisper_compute_host(melspec_ctx *ctx, const float *samples, size_t n_samples, size_t pad_to, float *out,
                                 size_t out_capacity_floats, int mel_major, size_t *n_frames);

/* The context's scratch only grows (pipeline buffers sized by the largest chunk, the precision guard's queue of 4 B per frame of
 * the largest batch, ragged plans, the raw rows of the melspec_whisper_* calls): this waits for the context's queued work and gives all
 * of it back.  The next call re-allocates. */
int melspec_release_scratch(melspec_ctx *ctx);
/* Pinned host memory (cudaMallocHost of src/cuda.rs:185-199): buffers from here skip the staging copy of the host calls. */
int melspec_host_alloc(void **p, size_t bytes);
int melspec_host_free(void *p);

/* ---- the GPUs of one node (additive: the reference binds one device, src/cuda.rs:246-247) ----------------------------
 * Every frame (Whisper) is independent, so clips are split into contiguous blocks per device, balanced by samples, and no
 * collective touches the data.  bounds[k] .. bounds[k+1] = the clips of shard k, k < n_shards. */
int melspec_shard_by_samples(const uint64_t *lengths, uint32_t n_clips, int n_shards, uint32_t *bounds /* [n_shards + 1] */);
/* One context + stream per listed device (devices == NULL: every gfx950 device; a device may be listed more than once). */
int melspec_sharded_create(melspec_sharded **out, const int *devices, int n_devices, int fft_size, int hop_size,
                           double sampling_rate, int n_mels);
void melspec_sharded_destroy(melspec_sharded *s);
int melspec_sharded_n_shards(const melspec_sharded *s);
melspec_ctx *melspec_sharded_ctx(melspec_sharded *s, int shard);   /* for device-resident work on one shard; owned by s */
/* melspec_compute_batch_host over all devices: one host thread per device drives that device's pipeline on its block of
 * clips; every shard writes its own part of `out`.  Synchronous. */
int melspec_sharded_compute_batch_host(melspec_sharded *s, const float *samples, const uint64_t *offsets, const uint64_t *lengths,
                                       uint32_t n_clips, float *out, const uint64_t *out_offsets, size_t out_capacity_floats,
                                       uint64_t *total_frames);
/* Device-resident shards: shard k's clips are on device k (d_pcm[k]), its frames stay there (d_out[k]); n_clips[k] clips per shard.
 * uniform: clip c of shard k = d_pcm[k] + c * clip_stride.  ragged: the clip tables of the shards one after the other (n_clips[0]
 * entries, then n_clips[1], ...), offsets relative to the shard's own d_pcm[k] / d_out[k]; h_out_offsets NULL = packed per shard.
 * Stream-ordered on every shard's context stream; melspec_sharded_synchronize waits for all shards.  No data crosses a device
 * boundary (per-clip split, no collective). */
int melspec_sharded_compute_uniform_device(melspec_sharded *s, const float *const *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                           const uint32_t *n_clips, float *const *d_out);
int melspec_sharded_compute_ragged_device(melspec_sharded *s, const float *const *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                          const uint32_t *n_clips, float *const *d_out, const uint64_t *h_out_offsets);
int melspec_sharded_synchronize(melspec_sharded *s);
/* Optional consolidation of device-resident results on one device: bytes[i] bytes at srcs[i] (device src_devices[i]) ->
 * dst + dst_offsets[i] bytes on dst_device, each piece on a stream of its source device (hipMemcpyPeerAsync: the pieces
 * cross their own xGMI links concurrently).  Synchronous; time it separately from the frames/s figure. */
int melspec_gather_peer(int dst_device, void *dst, const int *src_devices, const void *const *srcs, const size_t *bytes,
                        const size_t *dst_offsets, int n);

/* Additive surface (the reference has no multi-clip call): many equal-length clips in
 * one launch, PCM and output resident in HBM.  Clip c = d_pcm[c*clip_stride .. +clip_len).
 * d_out = [clip][frame][mel] f32, frames = melspec_num_frames(clip_len).
 * stream: hipStream_t (NULL = the context's own stream).  Asynchronous. */
int melspec_compute_uniform_device(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride,
                                   uint64_t clip_len, uint32_t n_clips, float *d_out, void *stream);

/* interleave_frames(frames, major_column_order, min_width) (src/mel.rs:480-544) fused into the
 * store: per clip the output is n_mels x W floats, W = melspec_interleaved_width(): the frame count,
 * +1 zero column if it is odd and min_width > 0 (whisper.cpp needs an even width), then zero columns up
 * to min_width (must be even).  major_column_order == 0 -> [mel][W] rows (what whisper.cpp's set_mel
 * takes); != 0 -> [W][mel] rows.  Clips with no frame are an error, like the reference's assert. */
size_t melspec_interleaved_width(const melspec_ctx *ctx, size_t n_samples, size_t min_width);
int melspec_compute_uniform_device_interleaved(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride,
                                               uint64_t clip_len, uint32_t n_clips, float *d_out,
                                               int major_column_order, uint64_t min_width, void *stream);

/* Ragged batch: clip c = d_pcm[h_offsets[c] .. + h_lengths[c]) (sample units, host arrays).
 * Output of clip c starts at d_out + h_out_offsets[c] (float units); pass NULL to pack the
 * clips back to back in order.  Clips shorter than fft_size produce zero frames. */
int melspec_compute_ragged_device(melspec_ctx *ctx, const float *d_pcm, const uint64_t *h_offsets,
                                  const uint64_t *h_lengths, uint32_t n_clips, float *d_out,
                                  const uint64_t *h_out_offsets, void *stream);

/* The same batch with its clip table in DEVICE memory (a segmenter or VAD on the GPU produces it; nothing is copied back):
 * d_offsets / d_lengths in samples, d_out_offsets in floats (NULL: the clips' frames packed back to back in clip order).  The plan
 * the host would build is built by a kernel on `stream`.  max_total_frames: an upper bound of the frames of all clips together (the
 * capacity of d_out in frames) -- it sizes the launch and the scratch; the true count stays on the device.  Asynchronous. */
int melspec_compute_ragged_device_desc(melspec_ctx *ctx, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                       uint32_t n_clips, float *d_out, const uint64_t *d_out_offsets, uint64_t max_total_frames,
                                       void *stream);

/* ---- 16-bit ends: int16 PCM in, f16 / bf16 rows out --------------------------------------------------------------------------
 * Audio arrives as 16-bit PCM (the reference's own example converts by hand, examples/vad_ten_eval/src/main.rs:298-299:
 * `sample as f32 / 32768.0`) and the encoders behind the rows run in f16 or bf16.  These calls read and write those types in
 * the kernel's own load and store: no conversion pass, half the bytes each way.
 *   MELSPEC_PCM_S16: the sample's value is int16 * 2^-15, exactly -- the call gives the bits of the f32 call on the batch
 *   converted by `v as f32 / 32768.0`.  MELSPEC_OUT_F16 / _BF16: the f32 row value rounded to nearest even.
 * Strides, offsets, lengths and capacities count ELEMENTS (samples in, row values out), never bytes; only natural alignment
 * of the element type is required (a ragged int16 clip may start at an odd sample, an f16 output at an odd element).
 * Everything else -- frame count, short clips, stream ordering, precision modes, error codes -- is that of
 * melspec_compute_uniform_device / _ragged_device / _host.  (F32, F32) is always supported and is the existing path.  The
 * other five combinations are computed by the contexts of melspec_create(.., 400, hop, 16000, n_mels) with Whisper's 80- or
 * 128-mel bank (melspec_supports_io == 1); every other context returns MELSPEC_ERR_UNSUPPORTED and does not touch the output. */
#define MELSPEC_PCM_F32  0
#define MELSPEC_PCM_S16  1      /* int16_t, value = sample * 2^-15 exactly */
#define MELSPEC_OUT_F32  0
#define MELSPEC_OUT_F16  1      /* IEEE binary16, round to nearest even of the f32 row value */
#define MELSPEC_OUT_BF16 2      /* bfloat16, round to nearest even; a NaN stays a NaN */
/* 1 if this context computes (pcm_dtype, out_dtype) batches, 0 if not (then the calls below return MELSPEC_ERR_UNSUPPORTED). */
int melspec_supports_io(const melspec_ctx *ctx, int pcm_dtype, int out_dtype);
int melspec_compute_uniform_device_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                      uint32_t n_clips, void *d_out, int out_dtype, void *stream);
int melspec_compute_ragged_device_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                     const uint64_t *h_lengths, uint32_t n_clips, void *d_out, int out_dtype,
                                     const uint64_t *h_out_offsets, void *stream);
/* melspec_compute_host with 16-bit ends: the int16 bytes are what crosses the bus, and so are the 16-bit rows. */
int melspec_compute_host_io(melspec_ctx *ctx, const void *samples, int pcm_dtype, size_t n_samples,
                            void *out, int out_dtype, size_t out_capacity_elems, size_t *n_frames);

/* The centred Whisper features (the melspec_whisper_* calls above) with the same 16-bit ends.  Everything said there holds -- frame
 * count, pad / trim, precision modes and melspec_whisper_kernel_name, stream ordering, the context's scratch -- and everything said at
 * the top of this section: MELSPEC_PCM_S16 gives the bits of the f32 call on the batch converted by `v as f32 / 32768.0`, MELSPEC_OUT_F16 /
 * _BF16 the round-to-nearest-even of the f32 value the f32 call writes; strides, offsets, lengths and capacities count ELEMENTS; only the
 * natural alignment of the element type is required (an int16 clip may start at an odd sample, a 16-bit output at an odd element).
 *   Normalised calls: the raw rows and the clip maximum stay f32 in the context's scratch, the clamp runs in f32, and the value is rounded
 *   once, at the final store.
 *   Split calls: d_rows holds the raw log10 values in out_dtype; d_clip_max stays f32 and holds the bits of the f32 split call's -- the
 *   maximum is taken over the f32 values before rounding.  Rounding is monotone, so round(g) is the largest stored value of the clip.  A
 *   silent row is exactly -10 (representable in both 16-bit types); a clip without a frame writes only g = -10.
 * All six (pcm_dtype, out_dtype) combinations are computed on the contexts of melspec_whisper_supports (melspec_whisper_supports_io == 1);
 * (F32, F32) is the f32 call: same kernels, same bits.  Every other context returns MELSPEC_ERR_UNSUPPORTED and leaves its output untouched.
 * Statuses: an unknown dtype code is MELSPEC_ERR_INVALID_ARG, checked right after the NULL context; a d_pcm, d_out or d_rows that is not
 * aligned to its element type is MELSPEC_ERR_INVALID_ARG, checked with the device pointers; everything else is the f32 calls' order.
 * NOT covered: a device-resident clip table with pad_to == 0 (the _desc calls need a fixed width); the sharded object; the stream bank. */
int melspec_whisper_supports_io(const melspec_ctx *ctx, int pcm_dtype, int out_dtype);
int melspec_whisper_compute_uniform_device_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                              uint32_t n_clips, uint64_t pad_to, void *d_out, int out_dtype, int mel_major, void *stream);
int melspec_whisper_compute_ragged_device_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                             const uint64_t *h_lengths, uint32_t n_clips, uint64_t pad_to, void *d_out, int out_dtype,
                                             const uint64_t *h_out_offsets, int mel_major, void *stream);
int melspec_whisper_compute_uniform_device_split_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                                    uint32_t n_clips, uint64_t pad_to, void *d_rows, int out_dtype, float *d_clip_max,
                                                    void *stream);
int melspec_whisper_compute_ragged_device_split_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                                   const uint64_t *h_lengths, uint32_t n_clips, uint64_t pad_to, void *d_rows, int out_dtype,
                                                   const uint64_t *h_rows_offsets, float *d_clip_max, void *stream);
/* One clip from host memory: the int16 bytes are what crosses the bus, and so are the 16-bit features.  out_capacity_elems >= T * n_mels. */
int melspec_whisper_compute_host_io(melspec_ctx *ctx, const void *samples, int pcm_dtype, size_t n_samples, size_t pad_to, void *out,
                                    int out_dtype, size_t out_capacity_elems, int mel_major, size_t *n_frames);

/* ---- the centred Whisper features from a clip table in device memory ----------------------------------------------------------------
 * The four ragged calls above with every h_ table replaced by a device array: d_offsets / d_lengths [n_clips] count samples (elements of
 * the PCM type), d_out_offsets / d_rows_offsets count output elements (NULL: packed in clip order).  A kernel on `stream` reads them and
 * builds the plan -- a VAD or segmenter on the GPU hands its segment table over without a copy to the host.  The host never reads a table
 * and never waits for the call's stream; the tables are read in stream order and must stay valid until the call's work has run.  The
 * context's plan and scratch buffers are used in stream order: a call on another stream than the context's previous call first waits for
 * that previous stream, as every call that uses the context's scratch does.  The result is,
 * bit for bit, what the host-table call writes for the same tables: every mode, bank, layout and dtype pair, steps 1 - 6 above,
 * element-counted offsets and natural alignment unchanged.
 * pad_to must be at least 400 (0 is MELSPEC_ERR_INVALID_ARG: without a fixed width the frame count of a clip is known only on the
 * device): every clip has T = pad_to / 160 frames, so the output holds n_clips * T * n_mels elements and the call needs no bound of the
 * caller's.  A length above pad_to is trimmed, a length of 0 is an all-silent clip; no length is rejected and no sample at or past
 * min(length, pad_to) of a clip is read.
 * Statuses, in this order: NULL context; (_io) the dtype codes; an unsupported context (MELSPEC_ERR_UNSUPPORTED, the contexts of
 * melspec_whisper_supports); pad_to; n_clips == 0 (OK, nothing queued); NULL d_offsets / d_lengths; NULL d_pcm / destination; (split)
 * NULL d_clip_max; (_io) alignment to the element type; more than 0xffffffff / 5 clips (MELSPEC_ERR_INVALID_ARG).  A refused call queues
 * nothing and writes nothing.  Growing the context's scratch may allocate; a second call of the same size allocates nothing. */
int melspec_whisper_supports_desc(const melspec_ctx *ctx);
int melspec_whisper_compute_ragged_device_desc(melspec_ctx *ctx, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                               uint32_t n_clips, uint64_t pad_to, float *d_out, const uint64_t *d_out_offsets, int mel_major,
                                               void *stream);
int melspec_whisper_compute_ragged_device_desc_split(melspec_ctx *ctx, const float *d_pcm, const uint64_t *d_offsets,
                                                     const uint64_t *d_lengths, uint32_t n_clips, uint64_t pad_to, float *d_rows,
                                                     const uint64_t *d_rows_offsets, float *d_clip_max, void *stream);
int melspec_whisper_compute_ragged_device_desc_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, const uint64_t *d_offsets,
                                                  const uint64_t *d_lengths, uint32_t n_clips, uint64_t pad_to, void *d_out, int out_dtype,
                                                  const uint64_t *d_out_offsets, int mel_major, void *stream);
int melspec_whisper_compute_ragged_device_desc_split_io(melspec_ctx *ctx, const void *d_pcm, int pcm_dtype, const uint64_t *d_offsets,
                                                        const uint64_t *d_lengths, uint32_t n_clips, uint64_t pad_to, void *d_rows,
                                                        int out_dtype, const uint64_t *d_rows_offsets, float *d_clip_max, void *stream);

/* Benchmark helper (the reference's #[ignore] Instant-timed benches, src/cuda.rs:547-613): runs
 * `warmup` untimed and `iters` timed melspec_compute_uniform_device calls on the context's own
 * stream between two HIP events and returns the average milliseconds per call. */
int melspec_time_uniform_device(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride,
                                uint64_t clip_len, uint32_t n_clips, float *d_out,
                                int warmup, int iters, float *avg_ms);

/* The same calls with a HIP event pair around the FIRST kernel of every call -- in AUTO the f32 kernel, without the gated f64 launch
 * behind it -- and the average of those pairs: the launch duration of the dominant kernel, as a profiler's kernel trace reports it
 * (bench.py's roofline.achieved).  Fused f32 n_fft = 400 contexts only. */
int melspec_time_first_kernel(melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips, float *d_out,
                              int warmup, int iters, float *avg_first_kernel_ms);

/* Wait for everything this context has queued on `stream` (cudaStreamSynchronize, src/cuda.rs:129). */
int melspec_synchronize(melspec_ctx *ctx, void *stream);

/* ---- the stand-alone mel helpers: SparseMelFilterbank, log_mel_spectrogram, norm_mel (src/mel.rs:40-168, 436-469) ----------
 * For callers that keep the reference's split API (examples/vad_ten_eval/src/main.rs:232-256: compute_all_cpu -> their own bank).
 * dtype: MELSPEC_STFT_F32 / MELSPEC_STFT_F64 (element type of the arrays).  The sums are the reference's left folds over its sparse
 * rows with a separate multiply and add: project_power is bit-exact against the f32 / f64 reference arithmetic. */
typedef struct melspec_bank melspec_bank;
/* SparseMelFilterbank::from_dense (src/mel.rs:48-71) / from_mel (:73-87) */
int melspec_bank_from_dense(melspec_bank **out, int device, const double *filters, int n_mels, int fft_bins);
int melspec_bank_from_mel(melspec_bank **out, int device, double sample_rate, int n_fft, int n_mels, double f_min, double f_max,
                          int htk, int norm);
void melspec_bank_destroy(melspec_bank *bank);
int melspec_bank_n_mels(const melspec_bank *bank);              /* n_mels()            src/mel.rs:89-91  */
int melspec_bank_fft_bins(const melspec_bank *bank);            /* fft_bins()          src/mel.rs:93-95  */
int melspec_bank_non_zero_weights(const melspec_bank *bank);    /* non_zero_weights()  src/mel.rs:97-99  */
/* weights_for_mel(mel_idx) (src/mel.rs:102-104): the row's SparseMelWeight { bin, weight } entries in ascending bin order, at most
 * `capacity` of them copied; returns the row's entry count (-1: bad index).  bins / weights may be NULL. */
int melspec_bank_weights_for_mel(const melspec_bank *bank, int mel_idx, int *bins, double *weights, int capacity);
/* project_power_f64 / project_power_f32 (src/mel.rs:106-146) for n_frames rows: power [n_frames][fft_bins] -> [n_frames][n_mels] */
int melspec_bank_project_power_device(melspec_bank *bank, const void *d_power, int dtype, uint64_t n_frames, void *d_out, void *stream);
int melspec_bank_project_power_host(melspec_bank *bank, const void *power, int dtype, size_t n_frames, void *out);
/* log_mel_spectrogram(stft, mel_filters) (src/mel.rs:436-441 -> project_stft_log10 :148-168) for n_frames frames: complex frames
 * [n_frames][n_fft] (interleaved re, im; what compute_all_cpu / melspec_stft_* with full = 1 return) -> log10(max(E, 1e-10)),
 * [n_frames][n_mels] f64, NOT normalised (norm_mel below). */
int melspec_bank_log_mel_device(melspec_bank *bank, const void *d_stft, int dtype, int n_fft, uint64_t n_frames, double *d_out, void *stream);
int melspec_bank_log_mel_host(melspec_bank *bank, const void *stft, int dtype, int n_fft, size_t n_frames, double *out);
/* norm_mel (f64, src/mel.rs:448-454) / norm_mel_vec (f32, :457-469): ONE maximum over the n_values given (a frame, a window of
 * frames, a whole clip: "flexibility in the sample size that's normalised over"), then (max(x, mmax - 8) + 4) / 4. */
int melspec_bank_norm_mel_device(melspec_bank *bank, const void *d_in, int dtype, uint64_t n_values, void *d_out, void *stream);
int melspec_bank_norm_mel_host(melspec_bank *bank, const void *in, int dtype, size_t n_values, void *out);

/* ---- host-side table builders (pure CPU, usable without a GPU) --------------------- */

/* mel(sr, n_fft, n_mels, f_min, f_max, htk, norm) (src/mel.rs:547-589): dense row-major
 * [n_mels][n_fft/2+1] f64.  f_min < 0 == None (0 Hz); f_max <= 0 == None (sr/2).
 * Pinned by testdata/mel_filters.npz @1e-7 (src/mel.rs:838-850). */
int melspec_mel_filterbank(double sr, int n_fft, int n_mels, double f_min, double f_max,
                           int htk, int norm, double *out);
/* hann_window (src/stft.rs:141-145), periodic, f64. */
int melspec_hann_window(int n, double *out);
/* hz_to_mel / mel_to_hz / mel_frequencies / fft_frequencies (src/mel.rs:591-643): the scale the filterbank above is built on
 * (Slaney, or HTK when htk != 0); mel_frequencies fills n_mels values, fft_frequencies n_fft/2 + 1.  Host only. */
double melspec_hz_to_mel(double frequency, int htk);
double melspec_mel_to_hz(double mel, int htk);
int melspec_mel_frequencies(int n_mels, double fmin, double fmax, int htk, double *out);
int melspec_fft_frequencies(double sr, int n_fft, double *out);
/* kaldi_mel_filterbank (src/fbank.rs:253-301): dense [num_mel_bins][fft_size/2+1] f64. */
int melspec_kaldi_mel_filterbank(double sample_rate, int fft_size, int num_mel_bins,
                                 double low_freq, double high_freq, double *out);

/* ---- Kaldi fbank: replaces Fbank (src/fbank.rs:85-247) ------------------------------ */

/* FbankConfig (src/fbank.rs:25-64); `dither` and `use_energy` exist in the reference
 * struct but are never read by Fbank::compute, so they are not carried. */
typedef struct melspec_fbank_config {
    double sample_rate;       /* 16000.0 */
    int32_t num_mel_bins;     /* 80 */
    double frame_length_ms;   /* 25.0 */
    double frame_shift_ms;    /* 10.0 */
    double energy_floor;      /* 0.0 -> FLT_EPSILON (src/fbank.rs:210-214) */
    int32_t use_log_fbank;    /* 1 */
    int32_t use_power;        /* 1 */
    double preemphasis;       /* 0.97 */
    int32_t apply_cmn;        /* 1 */
    double low_freq;          /* 20.0 */
    double high_freq;         /* 0.0 == Nyquist */
} melspec_fbank_config;

void melspec_fbank_default_config(melspec_fbank_config *cfg);          /* FbankConfig::default (src/fbank.rs:46-64) */
int melspec_fbank_create(melspec_fbank **out, int device, const melspec_fbank_config *cfg); /* Fbank::new (src/fbank.rs:94-132) */
void melspec_fbank_destroy(melspec_fbank *fb);
size_t melspec_fbank_num_frames(const melspec_fbank *fb, size_t n_samples); /* src/fbank.rs:147-151 */
int melspec_fbank_num_mel_bins(const melspec_fbank *fb);
/* 1 if this configuration runs on the fused 512-point kernel, 0 if on the generic f64 kernel. */
int melspec_fbank_uses_fast_path(const melspec_fbank *fb);
/* on != 0: run this object on the any-geometry f64 path (an independent device path, kept as the on-device cross-check of the fused
 * kernel): 1 = whatever that path picks for the geometry (power-of-two frame sizes: pow2_frame_kernel), 2 = the workgroup-per-frame
 * kernel whatever the geometry (~60x slower than the fused kernel). */
int melspec_fbank_use_generic(melspec_fbank *fb, int on);
/* Fbank::compute(&self, samples) -> Array2<f32> (frames, num_mel_bins) (src/fbank.rs:141-236). */
int melspec_fbank_compute_host(melspec_fbank *fb, const float *samples, size_t n_samples,
                               float *out, size_t out_capacity_floats, size_t *n_frames);
/* Many equal-length clips, device resident; CMN (src/fbank.rs:224-233) is per clip. */
int melspec_fbank_compute_uniform_device(melspec_fbank *fb, const float *d_pcm, uint64_t clip_stride,
                                         uint64_t clip_len, uint32_t n_clips, float *d_out, void *stream);
/* Additive (round 6; the reference has one output contract, Fbank::compute, src/fbank.rs:141-236): the same batch as TWO outputs --
 * d_rows [clip][frame][num_mel_bins] as they are BEFORE the CMN of src/fbank.rs:224-233, and d_means [clip][num_mel_bins], the column
 * means that CMN subtracts (the fixed summation tree of the fused path: d_rows[c][f][m] - d_means[c][m] in f32 is, bit for bit, what
 * melspec_fbank_compute_uniform_device stores).  For a consumer that folds the subtraction into its own first read of the rows: the CMN's
 * second pass over them is a third of the fused kernel's memory traffic (profiles/r06_fbank_split.txt).  Needs FbankConfig::apply_cmn
 * (without it there are no means: MELSPEC_ERR_INVALID_ARG). */
int melspec_fbank_compute_uniform_device_split(melspec_fbank *fb, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                               uint32_t n_clips, float *d_rows, float *d_means, void *stream);
/* Fbank::compute for clips of any length in one launch (src/fbank.rs:141 is per clip): host or device clip tables, as
 * melspec_compute_ragged_device / _desc; offsets of the output in floats; CMN per clip. */
int melspec_fbank_compute_ragged_device(melspec_fbank *fb, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                        uint32_t n_clips, float *d_out, const uint64_t *h_out_offsets, void *stream);
int melspec_fbank_compute_ragged_device_desc(melspec_fbank *fb, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                             uint32_t n_clips, float *d_out, const uint64_t *d_out_offsets, uint64_t max_total_frames,
                                             void *stream);
/* Many host clips in one call (the reference calls Fbank::compute once per clip, src/fbank.rs:141): clip i = samples[offsets[i] ..
 * + lengths[i]) -> its [frames_i][num_mel_bins] rows at out + out_offsets[i] floats (NULL: packed in clip order).  Whole clips in
 * chunks through the pinned, double-buffered host pipeline (as melspec_compute_batch_host); pinned samples / out are used in place. */
int melspec_fbank_compute_batch_host(melspec_fbank *fb, const float *samples, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_clips,
                                     float *out, const uint64_t *out_offsets, size_t out_capacity_floats, uint64_t *total_frames);
/* As melspec_release_scratch: waits for the object's own stream and gives its grow-only scratch back (pipeline and staging buffers,
 * ragged plans); work queued on caller streams must have been synchronised by the caller. */
int melspec_fbank_release_scratch(melspec_fbank *fb);
int melspec_fbank_synchronize(melspec_fbank *fb, void *stream);

/* ---- 16-bit ends for the Kaldi fbank: int16 PCM in, f16 / bf16 features out --------------------------------------------------------
 * MELSPEC_PCM_* / MELSPEC_OUT_* as above, with the same meaning: a MELSPEC_PCM_S16 sample's value is int16 * 2^-15, exactly -- the
 * call gives the bits of the f32 call on the batch converted by `v as f32 / 32768.0`; DC removal, pre-emphasis and the Povey window
 * (src/fbank.rs:164-190) are applied to the converted samples with the roundings the f32 kernel has, the first-sample patch of
 * src/fbank.rs:172 included.  MELSPEC_OUT_F16 / _BF16: every element of [frame][num_mel_bins] is the f32 element the f32 call writes,
 * rounded to nearest even ONCE; a NaN stays a NaN, a value beyond the f16 range (possible with use_log_fbank = 0) becomes an infinity.
 * With apply_cmn the means are those of the f32 rows, from the fixed summation tree of the fused path, and only row - mean is rounded:
 * the fbank kernel writes its f32 rows into a scratch of the object (grow-only, frames * num_mel_bins * 4 bytes summed over the clips;
 * given back by melspec_fbank_release_scratch) and the CMN pass reads them there and writes the 16-bit rows to the caller.  Without
 * CMN there is no scratch and no second pass; (S16, F32) with CMN normalises the caller's f32 rows in place like the f32 call.
 * Strides, offsets, lengths and capacities count ELEMENTS, never bytes; only natural alignment of the element type is required (a
 * ragged int16 clip may start at an odd sample, a 16-bit clip output at an odd element).  Everything else -- frame count, clips
 * without a frame, stream ordering, error codes -- is that of melspec_fbank_compute_uniform_device / _ragged_device / _host.
 * (F32, F32) is always supported and is routed to the existing calls unchanged.  The other five combinations are computed by the
 * fused path with the compile-time 80-bin Kaldi bank (melspec_fbank_uses_fast_path == 1 and that bank: 16 kHz, 25 ms frames, 80 bins,
 * low_freq 20, high_freq Nyquist -- the default geometry; the frame shift, 10 ms by default, is a run-time value of the kernel and not
 * part of the condition) with any preemphasis, use_log_fbank, use_power, energy_floor and apply_cmn (melspec_fbank_supports_io == 1);
 * every other object -- other banks, other geometries, an object after melspec_fbank_use_generic(fb, on != 0) -- returns
 * MELSPEC_ERR_UNSUPPORTED, names its geometry in melspec_last_error and does not touch the output.  These calls always run the
 * two-kernel path (the wave-owned fbank kernel, then the CMN), never the workgroup-per-clip kernel the f32 call picks for large
 * uniform batches; the two paths give the same bits.
 * Measured on an MI355X at config 3 (1024 x 10 s, 80 bins, CMN on; tools/fbank_io_bench.py, profiles/fbank_io_dtypes.txt): (S16, F16)
 * 0.769 ms per call against 1.354 ms for the status quo it replaces (int16 -> f32 cast, the f32 call, f32 -> f16 cast): 1.76 x.  It does
 * not beat the f32 call itself (0.662 ms in the same run), which runs the single workgroup-per-clip kernel on that batch. */
int melspec_fbank_supports_io(const melspec_fbank *fb, int pcm_dtype, int out_dtype);
int melspec_fbank_compute_uniform_device_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                            uint32_t n_clips, void *d_out, int out_dtype, void *stream);
int melspec_fbank_compute_ragged_device_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                           const uint64_t *h_lengths, uint32_t n_clips, void *d_out, int out_dtype,
                                           const uint64_t *h_out_offsets, void *stream);
/* melspec_fbank_compute_host with 16-bit ends: the int16 bytes are what crosses the bus, and so are the 16-bit features. */
int melspec_fbank_compute_host_io(melspec_fbank *fb, const void *samples, int pcm_dtype, size_t n_samples,
                                  void *out, int out_dtype, size_t out_capacity_elems, size_t *n_frames);

/* ---- the Kaldi split output for ragged batches and with 16-bit ends: int16 PCM in, f16 / bf16 rows out, f32 means -------------------
 * melspec_fbank_compute_uniform_device_split (above) carried to what an ASR server in front of a Kaldi-style encoder has -- int16 PCM of
 * mixed lengths -- and wants -- half-precision features: 2 bytes read per sample, 2 bytes written per element, 4 * num_mel_bins bytes of
 * means per clip, no scratch rows and no second pass (the _io calls with CMN write f32 rows into a scratch and read them back).
 *   samples   MELSPEC_PCM_S16: int16 * 2^-15, exactly; the call behaves as on the batch converted by `v as f32 / 32768.0`.
 *   d_rows    clip c: [frames_c][num_mel_bins] at d_rows + h_rows_offsets[c] ELEMENTS (NULL: packed in clip order).  Every element is the
 *             f32 element an object with the same config and apply_cmn = 0 writes through melspec_fbank_compute_uniform_device /
 *             _ragged_device, rounded to nearest even ONCE (a NaN stays a NaN); for (., F32) rows those are its bits.
 *   d_means   [n_clips][num_mel_bins] f32, always packed: THE BITS melspec_fbank_compute_uniform_device_split gives for that clip alone
 *             -- the means of the f32 values by the fixed summation tree of the fused path, not of the rounded rows --, a function of
 *             the clip's samples and length only: not of its place in the batch, the other clips, the output offsets, the dtype
 *             combination or what ran before.  A clip without a frame has no rows and its mean slots are +0.0, as the uniform Kaldi split
 *             reports them (the NeMo split leaves such slots untouched; this one does not).
 * melspec_fbank_compute_ragged_device_split is the f32 form (f32 samples, f32 rows) and runs on every object with apply_cmn, by the
 * routing of melspec_fbank_compute_ragged_device: large batches on the workgroup-per-clip kernel, everything else on the wave kernel (or
 * the generic one) followed by the CMN pass, which then writes the means and leaves the rows -- both sum by the same tree.  For it,
 * d_rows[c][f][m] - d_means[c][m] in f32 is, bit for bit, what melspec_fbank_compute_ragged_device stores.
 * The _split_io calls take every valid (pcm, out) pair; (F32, F32) is handed to the f32 split calls as it is.  The other five run where
 * melspec_fbank_supports_split_io == 1: the condition of melspec_fbank_supports_io (the fused path with the compile-time 80-bin Kaldi
 * bank, not after melspec_fbank_use_generic) with use_power and apply_cmn on.  Checked in this order: NULL object; the dtype codes
 * (MELSPEC_ERR_INVALID_ARG); apply_cmn off (MELSPEC_ERR_INVALID_ARG, as the uniform split); an unsupported object
 * (MELSPEC_ERR_UNSUPPORTED, melspec_last_error names the geometry, no buffer touched); n_clips == 0 (OK); NULL tables; no frame in the
 * whole batch (OK; the mean slots are zeroed when d_means is given); NULL device pointers, NULL d_means; a pointer misaligned for its
 * element type (MELSPEC_ERR_INVALID_ARG).  Strides, offsets and capacities count ELEMENTS; natural alignment of the element type is
 * enough (a clip may start at an odd int16 sample, a clip's rows at an odd 16-bit element).  A clip of 2^31 frames or more returns
 * MELSPEC_ERR_UNSUPPORTED.  Stream-ordered and asynchronous; the tables are read before the call returns; the rows scratch of the _io
 * calls is never touched.
 * The 16-bit calls always run one kernel, fbank512_clip_split_io_kernel (csrc/fbank512_kaldi_split_io_kernels.hpp: the workgroup-per-clip
 * kernel with typed loads and stores, always in split mode; ten instantiations, none with scratch memory,
 * profiles/fbank_split_io_resources.txt), with one workgroup per clip at a time: a batch of fewer clips than the device has CUs is
 * correct but leaves CUs idle.
 * What it costs (MI355X, 1024 clips, 80 bins, ms per call + synchronise, median of 30 rounds, tools/fbank_split_io_bench.py,
 * profiles/fbank_split_io.txt; A: this call (S16, F16); B: melspec_fbank_compute_*_device_io (S16, F16) with CMN, the call A replaces;
 * C: the f32 split on f32 samples; D: torch int16 -> f32, C, torch f32 -> f16):
 *     config 3 (1024 x 10 s)     A 0.594   B 0.788   C 0.615   D 1.224     A / B 0.75   A / C 0.97   A / D 0.49
 *     ragged, 2-20 s per clip    A 0.682   B 0.996   C 0.700   D 1.389     A / B 0.68   A / C 0.97   A / D 0.49
 * The widest interquartile range of the rounds was 0.07 / 0.09 ms: A is below B and D beyond the spread, and NOT below C beyond it -- the
 * kernel is bound by its f64 instructions like fbank512_clip_kernel, and halving its bytes buys 3 %.  The gain is over the two-kernel
 * _io call and over the casts around the f32 split.
 * Not offered: a path over many CUs for a few long clips with 16-bit ends (use the f32 ragged split, which has one), and a device-table
 * (_desc) form of any Kaldi split. */
int melspec_fbank_supports_split_io(const melspec_fbank *fb, int pcm_dtype, int out_dtype);
int melspec_fbank_compute_ragged_device_split(melspec_fbank *fb, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                              uint32_t n_clips, float *d_rows, const uint64_t *h_rows_offsets, float *d_means, void *stream);
int melspec_fbank_compute_uniform_device_split_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                                  uint32_t n_clips, void *d_rows, int out_dtype, float *d_means, void *stream);
int melspec_fbank_compute_ragged_device_split_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                                 const uint64_t *h_lengths, uint32_t n_clips, void *d_rows, int out_dtype,
                                                 const uint64_t *h_rows_offsets, float *d_means, void *stream);
/* One clip from host memory: the int16 bytes go up, the 16-bit rows (capacity in elements; too small: MELSPEC_ERR_CAPACITY) and the
 * num_mel_bins means come back; *n_frames = the clip's frames. */
int melspec_fbank_compute_host_split_io(melspec_fbank *fb, const void *samples, int pcm_dtype, size_t n_samples, void *rows, int out_dtype,
                                        size_t rows_capacity_elems, float *means, size_t *n_frames);

/* ---- NeMo/Parakeet log-mel frontend: replaces BatchLogMelSpectrogram (src/mel.rs:171-418) ------- */

/* BatchLogMelConfig (src/mel.rs:171-208). */
typedef struct melspec_blm_config {
    int32_t sample_rate;            /* 16000 */
    int32_t n_fft;                  /* 512 */
    int32_t win_length;             /* 400 */
    int32_t hop_length;             /* 160 */
    int32_t n_mels;                 /* 80 */
    double f_min;                   /* 0.0 */
    double f_max;                   /* <= 0 == None (sample_rate / 2) */
    int32_t htk;                    /* 0 */
    int32_t norm;                   /* 1 */
    float preemphasis;              /* 0.0 (NeMo: 0.97) */
    int32_t center;                 /* 1 */
    float log_zero_guard;           /* f32::EPSILON (NeMo: 2^-24) */
    int32_t pad_to;                 /* 0 */
    int32_t normalize_per_feature;  /* 0 */
} melspec_blm_config;

typedef struct melspec_blm melspec_blm;
void melspec_blm_default_config(melspec_blm_config *cfg);                 /* BatchLogMelConfig::default (src/mel.rs:189-208) */
/* BatchLogMelSpectrogram::new (src/mel.rs:248-280); validate_batch_config's messages (src/mel.rs:656-683) come
 * back through melspec_last_error with MELSPEC_ERR_INVALID_ARG (== BatchLogMelError::InvalidConfig).
 * n_fft = 512 / win_length = 400 (the NeMo/Parakeet geometry) runs on the fused 512-point kernel, every other validated
 * config (n_fft <= 4096) on the generic f64 kernel (two orders of magnitude slower, same results). */
int melspec_blm_create(melspec_blm **out, int device, const melspec_blm_config *cfg);
void melspec_blm_destroy(melspec_blm *b);
size_t melspec_blm_num_frames(const melspec_blm *b, size_t n_samples);    /* valid frames (src/mel.rs:387-395) */
size_t melspec_blm_padded_frames(const melspec_blm *b, size_t n_samples); /* cols = pad_len(valid, pad_to) (src/mel.rs:751-756) */
/* compute_flat (src/mel.rs:304-385): feature-major [n_mels][cols] f32; *rows = n_mels, *cols = padded frames.
 * Empty input -> cols = 0 (src/mel.rs:326-332). */
int melspec_blm_compute_host(melspec_blm *b, const float *samples, size_t n_samples, float *out,
                             size_t out_capacity_floats, size_t *rows, size_t *cols);
/* Many equal-length clips resident in HBM; d_out = [clip][n_mels][cols]. */
int melspec_blm_compute_uniform_device(melspec_blm *b, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                       uint32_t n_clips, float *d_out, void *stream);
/* Clips of any length in one launch: clip c = d_pcm[h_offsets[c] .. + h_lengths[c]) -> [n_mels][cols_c] at d_out + h_out_offsets[c]
 * floats (NULL: packed in clip order), cols_c = melspec_blm_padded_frames(b, h_lengths[c]).  Fused kernel (n_fft 512 / win_length 400). */
int melspec_blm_compute_ragged_device(melspec_blm *b, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                      uint32_t n_clips, float *d_out, const uint64_t *h_out_offsets, void *stream);
/* The same batch with its clip table in DEVICE memory (a segmenter or VAD on the GPU produces it; nothing is copied back), as
 * melspec_compute_ragged_device_desc and melspec_fbank_compute_ragged_device_desc: d_offsets / d_lengths in samples, d_out_offsets in
 * floats (NULL: the clips' rows packed back to back in clip order).  Clip c = d_pcm[d_offsets[c] .. + d_lengths[c]) -> [n_mels][cols_c]
 * f32 at d_out + d_out_offsets[c], cols_c = melspec_blm_padded_frames(len_c), normalised or not as the context's normalize_per_feature
 * says.  The plan the host would build -- centred or plain frame counts, the pad_to rounding, the clips' lengths and valid frames, the
 * normaliser's counter -- is built by one kernel on `stream`; the call reads no host table, queues no copy between host and device, and
 * synchronises only when its plan buffer has to grow or was last used on another stream.  Everything else is stream-ordered and
 * asynchronous.  Supported where the ragged call is: the fused geometry, n_fft 512 / win_length 400 (melspec_blm_supports_desc == 1).
 * For every accepted clip the output is THE BITS melspec_blm_compute_ragged_device writes for the same tables on the host, in the same
 * precision mode, whatever the two bounds, the clip's place in the batch, the other clips or what ran before.  (The normaliser's launch
 * is sized from max_clip_samples; the order of a row's sum of squares, which depends on the batch's longest clip in the host-table call,
 * is noted by the planner kernel from the true lengths and followed whatever the launch's size.)
 * The two bounds exist so that nothing the launch sizes from the host can be overrun by what the device table says:
 *   max_clip_samples   sizes the normaliser (its LDS rows hold the valid frames of a clip that long; a bound that does not fit LDS runs
 *                      the one-thread-per-row pass);
 *   max_total_columns  sizes the grid and the block table: an upper bound of the sum of cols_c -- with packed outputs, the capacity of
 *                      d_out in columns.
 * Rejection is decided by the planner kernel: (A) a clip with len > max_clip_samples is rejected and planned as a clip of length 0 -- no
 * rows, no space in a packed output, none of its samples read; (B) if the columns of the clips that survive (A) sum to more than
 * max_total_columns, every clip is rejected and nothing is written to d_out.  d_rejected (device, may be NULL) receives the number of
 * rejected clips, 0 .. n_clips; every call that launches writes it.
 * Checked in this order: NULL context (INVALID_ARG, "blm is NULL"); a context off the fused kernel (UNSUPPORTED, the ragged call's
 * message); n_clips == 0 or a bound of 0 (OK, nothing queued, d_rejected untouched); NULL d_pcm / d_out / d_offsets / d_lengths
 * (INVALID_ARG); max_total_columns >= 2^40 or a max_clip_samples whose row has 2^31 columns or more (UNSUPPORTED: the plan's integer
 * widths).
 * What it costs (1024 clips of 2-20 s, ms per call + synchronise, profiles/blm_desc.txt; A: this call with the tables resident on the
 * device, B: what it replaces -- the two tables copied to the host with a synchronise, then melspec_blm_compute_ragged_device --,
 * C: melspec_blm_compute_ragged_device with the tables already on the host), 80 / 128 mels, both precision modes, normalisation off and
 * on: A takes 0.92-0.97 x the time of B (about 0.04 ms less per call: the two copies and their synchronise) and 0.97-1.00 x of C -- the
 * planner kernel costs what C's host-side plan and its two small uploads cost.  What the call saves a pipeline is the synchronise
 * itself, which this figure counts only as time.
 * Not offered: a _desc form of the split output (its rounds wait for every wave of the workgroup -- "a round with a wave missing would
 * never end", blm_stats_plan.hpp -- so a unit count that only the device knows needs a design of its own); _desc with int16 PCM in or
 * 16-bit rows out. */
int melspec_blm_supports_desc(const melspec_blm *b);     /* 1: the fused geometry (n_fft 512 / win_length 400), as the ragged call */
int melspec_blm_compute_ragged_device_desc(melspec_blm *b, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                           uint32_t n_clips, float *d_out, const uint64_t *d_out_offsets, uint64_t max_total_columns,
                                           uint64_t max_clip_samples, uint32_t *d_rejected, void *stream);
/* The same from host memory, many clips per call (BatchLogMelSpectrogram::compute is per clip, src/mel.rs:299): clip i ->
 * [n_mels][cols_i] at out + out_offsets[i] floats (NULL: packed); *total_columns = sum of cols_i.  Host pipeline as above. */
int melspec_blm_compute_batch_host(melspec_blm *b, const float *samples, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_clips,
                                   float *out, const uint64_t *out_offsets, size_t out_capacity_floats, uint64_t *total_columns);
int melspec_blm_release_scratch(melspec_blm *b);   /* as melspec_fbank_release_scratch */

/* ---- 16-bit ends for this frontend: int16 PCM in, f16 / bf16 features out ---------------------------------------------------------
 * MELSPEC_PCM_* / MELSPEC_OUT_* as above, with the same meaning: a MELSPEC_PCM_S16 sample's value is int16 * 2^-15, exactly -- the
 * call gives the bits of the f32 call on the batch converted by `v as f32 / 32768.0`, pre-emphasis (src/mel.rs:696-706) applied to the
 * converted f32 samples with the same two roundings.  MELSPEC_OUT_F16 / _BF16: every element of [n_mels][cols] -- the zero columns
 * from the valid frames up to cols (pad_to) included, a NaN staying a NaN -- is the f32 element the f32 call writes, rounded to nearest
 * even ONCE.  With normalize_per_feature the statistics are those of the f32 rows (f32 left-fold mean, unbiased variance, + 1e-5) and
 * only the final (v - mean) / sd is rounded: the mel kernel writes its f32 rows into a scratch of the context (grow-only,
 * n_clips * n_mels * cols * 4 bytes, ragged: summed over the clips; given back by melspec_blm_release_scratch) and the normaliser
 * reads them there and writes the 16-bit rows to the caller.  Without normalisation there is no scratch and no second pass.
 * Strides, offsets, lengths and capacities count ELEMENTS, never bytes; only natural alignment of the element type is required (a
 * ragged int16 clip may start at an odd sample, a 16-bit clip output at an odd element; mel rows start at odd elements whenever cols
 * is odd).  Everything else -- valid / padded frame counts, empty clips, stream ordering, precision modes, error codes -- is that of
 * melspec_blm_compute_uniform_device / _ragged_device / _host.  (F32, F32) is always supported and is the existing path.  The other
 * five combinations are computed by the fused geometry (n_fft 512 / win_length 400) with the 80- or 128-mel Slaney bank, in both
 * arithmetic modes and with any preemphasis, center, log_zero_guard, pad_to, normalize_per_feature (melspec_blm_supports_io == 1);
 * every other context returns MELSPEC_ERR_UNSUPPORTED and does not touch the output. */
int melspec_blm_supports_io(const melspec_blm *b, int pcm_dtype, int out_dtype);
int melspec_blm_compute_uniform_device_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                          uint32_t n_clips, void *d_out, int out_dtype, void *stream);
int melspec_blm_compute_ragged_device_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                         const uint64_t *h_lengths, uint32_t n_clips, void *d_out, int out_dtype,
                                         const uint64_t *h_out_offsets, void *stream);
/* melspec_blm_compute_host with 16-bit ends: the int16 bytes are what crosses the bus, and so are the 16-bit features. */
int melspec_blm_compute_host_io(melspec_blm *b, const void *samples, int pcm_dtype, size_t n_samples, void *out, int out_dtype,
                                size_t out_capacity_elems, size_t *rows, size_t *cols);

/* ---- split output for this frontend: un-normalised rows + per-feature mean and 1 / std ----------------------------------------------
 * normalize_per_feature (src/mel.rs:721-749) needs a row's mean and standard deviation, which are known only when the whole clip is
 * done: the normalised call therefore reads and rewrites every row a second time.  The split call returns what that pass would need
 * instead -- as melspec_fbank_compute_uniform_device_split does for the CMN -- and leaves (x - mean) * inv_std on the valid columns to a
 * consumer that can fold it into its own first read.
 *   d_rows    [clip][n_mels][cols] f32, cols = melspec_blm_padded_frames(clip_len): the un-normalised log-mel rows, zero past the valid
 *             frames -- the bits melspec_blm_compute_uniform_device writes from a context with the same config, normalize_per_feature
 *             = 0 and the same precision mode.  The context's own normalize_per_feature does not matter to this call.
 *   d_mean    [clip][n_mels] f32: the row's mean over its valid frames.
 *   d_inv_std [clip][n_mels] f32: 1 / (sqrt(var) + 1e-5), var the unbiased variance with the denominator max(valid - 1, 1); one valid
 *             frame gives var = 0 and inv_std = 1e5, as in the reference.
 * The statistics are accumulated next to the rows by the mel kernel (per block of 32 or 48 frames counted from the clip's first frame, in
 * f32 around the block's own mean) and merged per row in f64, rounded once: they are closer to the exact statistics of the returned rows
 * than the reference's f32 left folds (which the normalised call reproduces), and a function of the clip's samples, its length and the
 * precision mode only -- not of the clip's place in the batch, the batch's size or what the context ran before.  The partial sums live in
 * a scratch of the context (grow-only, n_clips * ceil(cols / 32) * n_mels * 8 bytes; melspec_blm_release_scratch gives it back).
 * What it costs today (1024 x 10 s, profiles/blm_split.txt): in MELSPEC_PRECISION_F32 the call takes 0.79-0.87 x the time of the
 * normalised call; in the default (f64) mode it is SLOWER than the normalised call (1.15-1.39 x) -- there the call saves the consumer's
 * own pass over the rows, not time inside this library.  Set the F32 mode where the call is used for speed.
 * A clip_len without a valid frame returns MELSPEC_OK and writes nothing.  Supported: the fused geometry (n_fft 512 / win_length 400)
 * with the 80- or 128-mel Slaney bank, both precision modes (melspec_blm_supports_split == 1; the condition of the 16-bit ends); every
 * other context returns MELSPEC_ERR_UNSUPPORTED, names its geometry in melspec_last_error and touches no buffer.  Uniform batches,
 * ragged batches (below) and the single host clip; these three calls take f32 samples and write f32 rows, the _split_io calls further
 * below have the 16-bit ends. */
int melspec_blm_supports_split(const melspec_blm *b);
int melspec_blm_compute_uniform_device_split(melspec_blm *b, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                             uint32_t n_clips, float *d_rows, float *d_mean, float *d_inv_std, void *stream);
/* The ragged form -- clips of any length in one launch, what an ASR server has: clip c = d_pcm[h_offsets[c] .. + h_lengths[c]) ->
 *   d_rows    [n_mels][cols_c] f32 at d_rows + h_rows_offsets[c] (floats; NULL: packed in clip order), cols_c = melspec_blm_padded_frames(len_c);
 *   d_mean, d_inv_std  [n_clips][n_mels] f32, always packed.
 * A clip's rows, mean and inv_std are THE BITS melspec_blm_compute_uniform_device_split gives for that clip alone in the same precision
 * mode, whatever the clip's place in the batch, the other clips, the batch's size, the output offsets or what ran before: every clip's
 * work is rounded up to whole rounds of the kernel's workgroup, so its blocks of 32 / 48 frames are counted from its own first frame.
 * A clip without a valid frame (length 0, or center = 0 and fewer than n_fft samples) has no rows, and its mean / inv_std slots are left
 * untouched; a batch without any valid frame returns MELSPEC_OK and writes nothing.  Checked in the order of
 * melspec_blm_compute_ragged_device: NULL context, an unsupported context (as above: MELSPEC_ERR_UNSUPPORTED, the same message, no buffer
 * touched), n_clips == 0 (OK), NULL tables, nothing to do (OK), NULL device pointers.  A batch with 2^32 blocks or more, or whose scratch
 * (blocks * n_mels * 8 bytes) does not fit size_t, returns MELSPEC_ERR_UNSUPPORTED ("too large for the split output's plan").  Stream-
 * ordered and asynchronous like the ragged call; the tables are read before the call returns.
 * What it costs (1024 clips of 2-20 s, profiles/blm_split_ragged.txt; A: this call, B: melspec_blm_compute_ragged_device without
 * normalize_per_feature, C: with it -- the call A replaces): in
 * MELSPEC_PRECISION_F32 A takes 0.74 x (80 mels) / 0.65 x (128 mels) the time of C and 1.16 x / 1.19 x of B; in the default (f64) mode
 * 0.96 x / 0.86 x of C and 1.37 x / 1.41 x of B.  A beats C in both modes there -- at 80 mels in f64 by 4 % only, a margin inside the
 * spread of the timed calls -- because the ragged normaliser is dearer than the uniform one, not because the f64 kernel got faster.
 * Not offered: a device-table (_desc) form of the split (the frontend's plain ragged call has one: melspec_blm_compute_ragged_device_desc);
 * the f64 kernel's known slowness (its per-round merge) is as it was. */
int melspec_blm_compute_ragged_device_split(melspec_blm *b, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                            uint32_t n_clips, float *d_rows, const uint64_t *h_rows_offsets, float *d_mean,
                                            float *d_inv_std, void *stream);
/* One clip from host memory: rows = [n_mels][cols] (capacity in floats), mean / inv_std = [n_mels]; *n_rows = n_mels, *n_cols = cols. */
int melspec_blm_compute_host_split(melspec_blm *b, const float *samples, size_t n_samples, float *rows, size_t rows_capacity_floats,
                                   float *mean, float *inv_std, size_t *n_rows, size_t *n_cols);
/* ---- the split output with 16-bit ends: int16 PCM in, f16 / bf16 rows out, f32 mean and 1 / std ----------------------------------------
 * The two contracts above joined, nothing new invented -- what a server that holds int16 PCM and wants half-precision features has been
 * building from parts: 2 bytes read per sample, 2 bytes written per element, no scratch rows and no second pass (the normalised _io call
 * writes f32 rows into a scratch and reads them back: about 800 of its 1120 bytes per frame at 80 mels).
 *   samples   MELSPEC_PCM_S16: int16 * 2^-15, exactly; the call behaves as the f32 split call on the batch converted by
 *             `v as f32 / 32768.0`, pre-emphasis applied to the converted samples.
 *   d_rows    every element is the element the f32 split call writes, rounded to nearest even ONCE (a NaN stays a NaN); pad columns are
 *             +0; pad columns and clips without a frame behave as in the f32 split calls.
 *   d_mean, d_inv_std  f32, packed [clip][n_mels]: THE BITS of the f32 split call -- the statistics of the f32 values, not of the rounded
 *             rows (as the normalised _io call defines its statistics) --, a function of the clip's samples, its length and the precision
 *             mode only.  A consumer's (row - mean) * inv_std therefore carries the row's rounding (half an ulp of the row type) times
 *             inv_std.
 * Strides, offsets and capacities count ELEMENTS; natural alignment of the element type is enough (a clip may start at an odd int16
 * sample, rows at an odd 16-bit element).  Supported where melspec_blm_supports_split is, for every valid (pcm, out) pair
 * (melspec_blm_supports_split_io == 1); (F32, F32) is handed to the f32 split calls as it is.  Checked in this order: NULL context, the
 * dtype codes (MELSPEC_ERR_INVALID_ARG), then the f32 split call's own checks in its order -- an unsupported context
 * (MELSPEC_ERR_UNSUPPORTED, the split call's message naming the geometry, no buffer touched), nothing to do (MELSPEC_OK), NULL tables /
 * pointers --, then a pointer misaligned for its element type (MELSPEC_ERR_INVALID_ARG).  Only the partials scratch of the f32 split
 * calls is used, in stream order; the rows scratch of the normalised _io call never is.  Stream-ordered and asynchronous like the f32
 * split calls.  One mel kernel serves the uniform and the ragged call (csrc/fbank512_stats_io_kernels.hpp); none of its twenty
 * instantiations uses scratch memory (profiles/blm_split_io_resources.txt).
 * What it costs (ms per call + synchronise, profiles/blm_split_io.txt; A: this call (S16, F16); B: melspec_blm_compute_*_io (S16, F16)
 * with normalize_per_feature = 1, the call A replaces; C: the f32 split call on f32 samples; D: torch int16 -> f32, C, torch f32 -> f16): 1024 x 10 s uniform / 1024 clips of 2-20 s ragged, 80 and 128 mels; the widest interquartile range of the rounds was 0.10-0.19 ms, so
 * differences below about 15 % are inside the spread.  MELSPEC_PRECISION_F32: A takes 0.87 x / 0.79 x (uniform, 80 / 128 mels) and
 * 0.73 x / 0.64 x (ragged) the time of B, 0.87-0.91 x of C and 0.42-0.45 x of D; beyond the spread that is "A below B" for the ragged
 * shapes and "A below D" everywhere, NOT for A against C or against the uniform B.  Default (f64) mode: on uniform batches A is SLOWER
 * than B, 1.50 x / 1.27 x -- the f64 stats kernel's per-round merge, as for the f32 split above --, ragged 1.00 x / 0.89 x; 0.94-0.98 x
 * of C; 0.57-0.62 x of D (below D beyond the spread everywhere).  Set the F32 mode where the call is used for speed; in f64 the call is
 * kept for its contract -- 16-bit rows with f32 statistics of the f32 values, and no rows scratch. */
int melspec_blm_supports_split_io(const melspec_blm *b, int pcm_dtype, int out_dtype);
int melspec_blm_compute_uniform_device_split_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                                uint32_t n_clips, void *d_rows, int out_dtype, float *d_mean, float *d_inv_std, void *stream);
int melspec_blm_compute_ragged_device_split_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                               const uint64_t *h_lengths, uint32_t n_clips, void *d_rows, int out_dtype,
                                               const uint64_t *h_rows_offsets, float *d_mean, float *d_inv_std, void *stream);
/* One clip from host memory: the int16 bytes go up, the 16-bit rows (capacity in elements) and the two f32 vectors come back. */
int melspec_blm_compute_host_split_io(melspec_blm *b, const void *samples, int pcm_dtype, size_t n_samples, void *rows, int out_dtype,
                                      size_t rows_capacity_elems, float *mean, float *inv_std, size_t *n_rows, size_t *n_cols);
/* Arithmetic of the fused kernel (n_fft 512 / win_length 400, 80 or 128 mels).  MELSPEC_PRECISION_F32: f32 window, FFT, power and
 * projection -- the reference's own arithmetic type for this frontend (src/mel.rs:251-252,356-357), as far from the f64 evaluation of
 * its definition as upstream's f32 code is (2.4e-4 on jfk_f32le.wav) at ~0.8 x the time.  AUTO (default) / F64: f64 up to |X|^2, within 1e-4
 * of that evaluation on every input.  melspec_blm_precision: what the next call will use (F32 or F64). */
int melspec_blm_set_precision(melspec_blm *b, int mode);
int melspec_blm_precision(const melspec_blm *b);
int melspec_blm_synchronize(melspec_blm *b, void *stream);

/* ---- streaming: Spectrogram::add + RingBuffer::maybe_mel (src/stft.rs:48-86, src/rb.rs:60-121) ---- */
/* A bank of n_streams independent live streams over one melspec_ctx (its geometry, tables and
 * kernels).  Per stream the device keeps what the reference keeps on the host: hop_buf's history (the
 * last n_fft - hop samples) and the samples accumulated towards the next hop (RingBuffer's
 * accumulated_samples); the host side of the handle keeps Spectrogram::idx.  A push appends a chunk of
 * any length <= max_chunk to each named stream and emits, per stream, exactly the frames the reference's
 * add_frame()/maybe_mel() loop would: one per completed hop once idx >= n_fft, so the first frame of a
 * stream starts at sample ceil(n_fft/hop)*hop - n_fft (80 for 400/160, 128 for 512/160) -- the alignment
 * testdata/rust_jfk_golden.npy pins (src/rb.rs:134-179).  Frames are computed in place on carry ++ chunk
 * by the batch kernels (no staging copy of the history), then the tail becomes the new carry.
 * The ctx must outlive the bank; one bank per host thread, like the ctx. */
typedef struct melspec_stream melspec_stream;

int melspec_stream_create(melspec_stream **out, melspec_ctx *ctx, uint32_t n_streams, uint32_t max_chunk);
void melspec_stream_destroy(melspec_stream *st);
/* Spectrogram::new state (zero history, idx = 0) for the listed streams; ids == NULL -> all. */
int melspec_stream_reset(melspec_stream *st, const uint32_t *ids, uint32_t n);
/* frames a push of n_new samples to stream id would emit now */
size_t melspec_stream_frames_after(const melspec_stream *st, uint32_t id, uint32_t n_new);

/* Host chunks: samples holds the n chunks back to back (lens[i] samples for stream ids[i], each id at most
 * once per call); out receives the emitted frames back to back in entry order ([frame][mel] each),
 * frames_out[i] how many entry i emitted.  Synchronous. */
int melspec_stream_push_host(melspec_stream *st, const uint32_t *ids, const float *samples, const uint32_t *lens, uint32_t n,
                             float *out, size_t out_capacity_floats, uint32_t *frames_out);
/* The same push emitting what Spectrogram::add itself returns (src/stft.rs:48-86): the spectrum of every completed frame,
 * [frame][bins] complex per entry (melspec_stft_bins; dtype MELSPEC_STFT_F32 / _F64), instead of its mel row. */
int melspec_stream_push_host_stft(melspec_stream *st, const uint32_t *ids, const float *samples, const uint32_t *lens, uint32_t n,
                                  void *out, size_t out_capacity_complex, uint32_t *frames_out, int dtype, int full);
/* Spectrogram::add with fewer than hop samples (src/stft.rs:57-60): the pending samples of each listed
 * stream are zero-padded to a hop, idx advances by the real samples only, at most one frame each. */
int melspec_stream_flush_host(melspec_stream *st, const uint32_t *ids, uint32_t n, float *out, size_t out_capacity_floats,
                              uint32_t *frames_out);
/* Device producers write the next chunk of stream id at melspec_stream_input_ptr(st, id) (fixed per
 * stream, 16-byte aligned, room for max_chunk samples) and then push lengths only.  Output goes to
 * d_out + out_offsets[i] floats (NULL -> back to back).  Returns after the launches have completed. */
float *melspec_stream_input_ptr(melspec_stream *st, uint32_t id);
int melspec_stream_push_device(melspec_stream *st, const uint32_t *ids, const uint32_t *lens, uint32_t n, float *d_out,
                               const uint64_t *out_offsets, uint32_t *frames_out, void *stream);

/* int16 PCM chunks in, f16 / bf16 rows out: the pushes above with typed ends (MELSPEC_PCM_* / MELSPEC_OUT_* as for the batch calls).
 * The bank's state stays f32.  A MELSPEC_PCM_S16 sample's value is int16 * 2^-15, exactly, converted where the chunk is copied into the
 * state: carry, history and every later frame are the bits the f32 bank holds after the same pushes of the converted chunks, for every
 * geometry a bank runs.  Rows of a MELSPEC_OUT_F16 / _BF16 push are the f32 rows the f32 push would emit for the same history, rounded
 * to nearest even once (a NaN stays a NaN), written by the frame kernels' own stores; they need melspec_supports_io(ctx,
 * MELSPEC_PCM_F32, out_dtype) -- the n_fft = 400 contexts with Whisper's 80- or 128-mel bank -- and the detector stage off (it reads
 * f32 rows): otherwise MELSPEC_ERR_UNSUPPORTED, melspec_last_error naming the geometry, nothing queued, the bank as it was.
 * Frame counts, first-frame alignment, flush, reset, error codes and "the launches have completed on return" are those of the f32
 * calls; capacities and offsets count elements of the row type, buffers need their element type's alignment only.  (F32, F32) is the
 * existing call.  Checked in this order: NULL bank, dtype codes, support, then what the f32 call checks.
 * melspec_stream_supports_io: 1 for any valid pcm_dtype with MELSPEC_OUT_F32; for _F16 / _BF16 what melspec_supports_io says of the ctx. */
int melspec_stream_supports_io(const melspec_stream *st, int pcm_dtype, int out_dtype);
int melspec_stream_push_host_io(melspec_stream *st, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n,
                                void *out, int out_dtype, size_t out_capacity_elems, uint32_t *frames_out);
int melspec_stream_flush_host_io(melspec_stream *st, const uint32_t *ids, uint32_t n, void *out, int out_dtype, size_t out_capacity_elems,
                                 uint32_t *frames_out);
/* d_chunks != NULL: chunk i is d_chunks[h_src_offsets[i] .. + lens[i]) in elements of pcm_dtype, anywhere in device memory
 * (h_src_offsets == NULL: back to back in entry order; an int16 chunk may start at an odd element); it is copied into the bank on
 * `stream`.  d_chunks == NULL: the chunks are already at melspec_stream_input_ptr, in f32 -- pcm_dtype must be MELSPEC_PCM_F32.
 * Rows go to d_out + out_offsets[i] elements of out_dtype (a 16-bit output may start at an odd element). */
int melspec_stream_push_device_io(melspec_stream *st, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets,
                                  const uint32_t *lens, uint32_t n, void *d_out, int out_dtype, const uint64_t *out_offsets,
                                  uint32_t *frames_out, void *stream);

/* ---- streaming Kaldi fbank: Fbank::compute (src/fbank.rs:141-236) fed chunk by chunk ---- */
/* A bank of n_streams independent streams over one melspec_fbank (its geometry, tables and kernels).  For each stream, after any
 * sequence of pushes whose chunks concatenate to x, the rows emitted so far are exactly the rows of Fbank::compute(x) with apply_cmn = 0:
 * frame k is emitted by the push that brings the stream to k * shift + frame_len samples -- no warm-up skip and no flush (the reference
 * drops the tail, and so does the bank).  The rows are the bits melspec_fbank_compute_host returns for x on an object with the same
 * config and apply_cmn = 0, however x was cut into chunks.  A push always emits rows BEFORE CMN, whatever the object's apply_cmn is
 * (the contract of melspec_fbank_compute_uniform_device_split carried over time); the bank keeps, per stream and mel bin, an f64 sum of
 * the emitted rows -- a left fold in frame order, so a function of the stream's samples alone -- and the frame count:
 * melspec_fbank_stream_stats_* return mean[bin] = (float)(sum / count) and count (zero means for count == 0).  At end of stream
 * rows - mean is the reference's CMN output to within its own f32 fold error; before that, online cumulative mean normalisation.
 * Per stream the device keeps the samples no emitted frame starts in (< frame_len) and, in front of them, the one sample the next
 * frame's pre-emphasis reads (src/fbank.rs:177-181: samples[start - 1]; the Povey window is 0 there, so it matters for non-finite
 * input only -- and there the rows follow the reference).  A stream that has emitted nothing has no such sample: what lay in its slot
 * before a reset never reaches its frame 0.
 * The handle is opaque and crosses the ABI as void *.  The fbank must outlive the bank; one bank per host thread, like the fbank.
 * Needs melspec_fbank_uses_fast_path(fb) == 1 and frame_shift <= frame_length: otherwise MELSPEC_ERR_UNSUPPORTED at create -- and at a
 * push after melspec_fbank_use_generic(fb, 1) -- with melspec_last_error naming the geometry.  n_streams == 0 or max_chunk == 0, a NULL
 * handle (no device is touched), an id out of range or twice in one push: MELSPEC_ERR_INVALID_ARG; a chunk longer than max_chunk:
 * MELSPEC_ERR_CAPACITY.  A push that fails leaves the bank, its state and its sums as they were. */
int melspec_fbank_stream_create(void **out, melspec_fbank *fb, uint32_t n_streams, uint32_t max_chunk);
void melspec_fbank_stream_destroy(void *st);
/* no history, no frames, zero sums for the listed streams; ids == NULL -> all */
int melspec_fbank_stream_reset(void *st, const uint32_t *ids, uint32_t n);
/* rows a push of n_new samples to stream id would emit now */
size_t melspec_fbank_stream_frames_after(const void *st, uint32_t id, uint32_t n_new);
/* Host chunks: samples holds the n chunks back to back (lens[i] elements of pcm_dtype -- MELSPEC_PCM_F32, or MELSPEC_PCM_S16 whose value is
 * int16 * 2^-15, exactly, converted where the chunk is copied into the f32 state -- for stream ids[i]); out receives the emitted rows
 * [frame][num_mel_bins] f32, back to back in entry order, frames_out[i] how many entry i emitted.  Synchronous. */
int melspec_fbank_stream_push_host(void *st, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n,
                                   float *out, size_t out_capacity_floats, uint32_t *frames_out);
/* Device producers: d_chunks != NULL: chunk i is d_chunks[h_src_offsets[i] .. + lens[i]) in elements of pcm_dtype (h_src_offsets == NULL:
 * back to back), copied into the bank on `stream`; d_chunks == NULL: the chunks are already at melspec_fbank_stream_input_ptr(st, id)
 * (fixed per stream, 16-byte aligned, room for max_chunk samples), in f32.  Rows go to d_out + h_out_offsets[i] floats (NULL: back to
 * back).  The launches have completed on return, as for melspec_stream_push_device. */
float *melspec_fbank_stream_input_ptr(void *st, uint32_t id);
int melspec_fbank_stream_push_device(void *st, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets,
                                     const uint32_t *lens, uint32_t n, float *d_out, const uint64_t *h_out_offsets, uint32_t *frames_out,
                                     void *stream);
/* means: [n][num_mel_bins] f32 of the listed streams, counts: [n] rows emitted so far (may be NULL) */
int melspec_fbank_stream_stats_host(void *st, const uint32_t *ids, uint32_t n, float *means, uint64_t *counts);
int melspec_fbank_stream_stats_device(void *st, const uint32_t *ids, uint32_t n, float *d_means, uint64_t *h_counts, void *stream);

/* ---- streaming NeMo / Parakeet log-mel: BatchLogMelSpectrogram::compute (src/mel.rs) fed chunk by chunk ---- */
/* A bank of n_streams independent streams over one melspec_blm (its geometry, tables and kernels).  For each stream, after any sequence
 * of pushes whose chunks concatenate to x, followed by one finish, the columns emitted so far, concatenated in time, are exactly the
 * columns melspec_blm_compute_host returns for x from a context with the same config, normalize_per_feature = 0 and the same precision
 * mode (read at each push from melspec_blm_precision); pad_to is ignored.  Bit for bit, however x was cut into chunks.
 *   center = 1: frame k reads samples [k * hop - 200, k * hop + 200); a push emits it as soon as the stream holds k * hop + 200 samples,
 *     so every tap is a real sample.  finish emits the remaining frames up to k = total / hop with the reference's zero padding on the
 *     right (at most two per stream at the usual hops; in general the frames that overlap the last 200 samples) -- and nothing for a
 *     stream that never received a sample, as the reference returns no column for an empty input.
 *   center = 0: frame k exists once the stream holds k * hop + 512 samples (num_frames); finish emits nothing.
 * After finish the stream is ended: a push or a second finish returns MELSPEC_ERR_INVALID_ARG and leaves the bank as it was, the
 * statistics stay readable, reset starts the stream afresh.  Pre-emphasis follows the reference across chunk borders: sample 0 of a
 * stream is never pre-emphasised, every other sample uses its true predecessor (a NaN or an infinity there reaches the rows as in the
 * batch call); padding is zero after pre-emphasis.
 * A push always emits UN-NORMALISED rows, whatever the context's normalize_per_feature is (the contract of
 * melspec_blm_compute_uniform_device_split carried over time): entry i gets feature-major [n_mels][frames_i] f32.  Per stream and mel
 * row the bank keeps a running (count, mean, M2) in f64, updated one column at a time in time order (Welford: d = x - mean;
 * mean += d / count; M2 += d * (x - mean); every operation rounded once) -- a left fold over the stream's columns, so a function of the
 * stream's samples alone.  melspec_blm_stream_stats_* return mean[m] (f32), inv_std[m] = 1 / (sqrt(M2 / max(count - 1, 1)) + 1e-5) --
 * the split output's definition -- and the column count; count == 0 gives mean 0 and inv_std 1e5.  At end of stream (rows - mean) *
 * inv_std is the normalised call's output to within the error of its f32 folds; before that, online cumulative normalisation.
 * Per stream the device keeps the samples from the predecessor of the next frame's first tap on: fewer than 401 (center = 0: 457).
 * Rows of these calls are f32 (f16 / bf16 rows: the _io forms below); chunks are MELSPEC_PCM_F32 or MELSPEC_PCM_S16 (int16 * 2^-15,
 * exactly, converted where the chunk is copied into the f32 state).
 * The handle is opaque and crosses the ABI as void *.  The context must outlive the bank; one bank per host thread, like the context.
 * Needs the fused geometry (n_fft = 512, win_length = 400, a bank the fused kernels hold): otherwise MELSPEC_ERR_UNSUPPORTED at create
 * with melspec_last_error naming the geometry.  n_streams == 0 or max_chunk == 0, a NULL handle (no device is touched), an id out of
 * range or twice in one call: MELSPEC_ERR_INVALID_ARG; a chunk longer than max_chunk: MELSPEC_ERR_CAPACITY.  A call that fails leaves the
 * bank, its state and its statistics as they were.
 * Measured (profiles/blm_stream.txt; MI355X, 1024 live streams, ms per melspec_blm_stream_push_device at 10 ms / 100 ms / 1 s chunks):
 * f64 0.0545 / 0.0605 / 0.1484, MELSPEC_PRECISION_F32 0.0579 / 0.0592 / 0.1314.  In the same run the Kaldi bank's push took 0.0516 /
 * 0.0593 / 0.1317 ms and melspec_blm_compute_ragged_device on the history ++ chunk batch (which leaves the history, the batch and the
 * statistics to its caller) 0.0370 / 0.0433 / 0.0958 ms (F32: 0.0384 / 0.0406 / 0.0795): the bank is 1.40 - 1.65 x SLOWER than that call. */
int melspec_blm_stream_create(void **out, melspec_blm *b, uint32_t n_streams, uint32_t max_chunk);
void melspec_blm_stream_destroy(void *st);
/* no history, no frames, not ended, zero statistics for the listed streams; ids == NULL -> all.  A bad id: nothing is reset. */
int melspec_blm_stream_reset(void *st, const uint32_t *ids, uint32_t n);
/* columns a push of n_new samples to stream id would emit now / a finish of it would (0 for an ended stream) */
size_t melspec_blm_stream_frames_after(const void *st, uint32_t id, uint32_t n_new);
size_t melspec_blm_stream_finish_frames(const void *st, uint32_t id);
/* Host chunks: samples holds the n chunks back to back (lens[i] elements of pcm_dtype for stream ids[i]); out receives the emitted
 * rows, [n_mels][frames_out[i]] f32 per entry, back to back in entry order.  Synchronous. */
int melspec_blm_stream_push_host(void *st, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n,
                                 float *out, size_t out_capacity_floats, uint32_t *frames_out);
/* Device producers: d_chunks != NULL: chunk i is d_chunks[h_src_offsets[i] .. + lens[i]) in elements of pcm_dtype (h_src_offsets == NULL:
 * back to back), copied into the bank on `stream`; d_chunks == NULL: the chunks are already at melspec_blm_stream_input_ptr(st, id)
 * (fixed per stream, 16-byte aligned, room for max_chunk samples), in f32.  Entry i's rows go to d_out + h_out_offsets[i] floats (NULL:
 * back to back).  The launches have completed on return, as for melspec_stream_push_device. */
float *melspec_blm_stream_input_ptr(void *st, uint32_t id);
int melspec_blm_stream_push_device(void *st, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets,
                                   const uint32_t *lens, uint32_t n, float *d_out, const uint64_t *h_out_offsets, uint32_t *frames_out,
                                   void *stream);
/* end of the listed streams: the frames that read past the stream's end, laid out like a push's */
int melspec_blm_stream_finish_host(void *st, const uint32_t *ids, uint32_t n, float *out, size_t out_capacity_floats, uint32_t *frames_out);
int melspec_blm_stream_finish_device(void *st, const uint32_t *ids, uint32_t n, float *d_out, const uint64_t *h_out_offsets,
                                     uint32_t *frames_out, void *stream);
/* mean, inv_std: [n][n_mels] f32 of the listed streams, counts: [n] columns emitted so far (may be NULL) */
int melspec_blm_stream_stats_host(void *st, const uint32_t *ids, uint32_t n, float *mean, float *inv_std, uint64_t *counts);
int melspec_blm_stream_stats_device(void *st, const uint32_t *ids, uint32_t n, float *d_mean, float *d_inv_std, uint64_t *h_counts,
                                    void *stream);

/* ---- f16 / bf16 rows out of the two stream banks above: their pushes (and the NeMo bank's finish) with typed ends ---- */
/* pcm_dtype is MELSPEC_PCM_F32 or MELSPEC_PCM_S16, out_dtype MELSPEC_OUT_F32, _F16 or _BF16, as for the batch calls.
 * Rows: an element of a MELSPEC_OUT_F16 / _BF16 call is the f32 element the f32 call would emit for the same bank history, rounded to
 * nearest even once; a NaN stays a NaN, a value beyond the f16 range becomes an infinity.  Layouts are the f32 calls': Kaldi
 * [frame][num_mel_bins] per entry, NeMo [n_mels][frames_i] per entry, and for the NeMo bank's finish the zero-padded last columns laid
 * out the same way.
 * State and statistics are untouched by the row type: after any mix of f32 and typed calls the bank's carry, its frame counts and what
 * melspec_fbank_stream_stats_* / melspec_blm_stream_stats_* return are the bits a bank driven through the f32 calls alone holds.  The
 * statistics are folds over the f32 rows; the rounded rows never feed them.  How: the frame kernels of the f32 push, unchanged, write their
 * f32 rows packed into a scratch of the bank (grow-only, allocated by the first typed call -- a bank that only sees f32 calls never has
 * one --, released at destroy), and a twin of the fold kernel behind them reads each f32 element there once, folds it exactly as the f32
 * push's fold does (same operations, same order, no contraction) and stores it, rounded, at its place in the caller's rows
 * (csrc/stream_banks_io_kernels.hpp; the precedent is the batch _io calls with CMN / normalize_per_feature above).  No kernel reads the
 * caller's rows and there is no conversion pass.  Because the frame kernels are the f32 push's, typed rows exist on every geometry a bank
 * can be created on -- not only on the narrower set of the batch _io calls: melspec_*_stream_supports_io is 1 for every valid pair of
 * codes on a live bank whose object is still on the fused path, 0 otherwise (NULL or foreign handle, unknown code).
 * Capacities and offsets count elements of the row type; buffers need the natural alignment of their element type only.  A 16-bit entry
 * may start at an odd element, and in the NeMo layout every mel row behind the first does whenever frames_i is odd: neighbouring entries
 * may share a 4-byte word.  Rows are written with one 2-byte store per element, never with a read-modify-write of a word.
 * (pcm, MELSPEC_OUT_F32) is the existing call: the same launches, no scratch.
 * Checked in this order: NULL bank (MELSPEC_ERR_INVALID_ARG, no device is touched, melspec_last_error says "NULL"), unknown pcm_dtype /
 * out_dtype code (MELSPEC_ERR_INVALID_ARG), support (MELSPEC_ERR_UNSUPPORTED), then everything the f32 call checks, with its codes:
 * d_chunks == NULL needs MELSPEC_PCM_F32, a device pointer misaligned for its element type, an id out of range or listed twice,
 * MELSPEC_ERR_CAPACITY, an ended NeMo stream.  A refused call queues nothing, writes nothing to the output and leaves the bank, its
 * state and its statistics as they were.  "The launches have completed on return" holds as for the f32 pushes.  The host forms move the
 * rows across the bus in their own type.
 * Measured (profiles/stream_banks_io.txt; MI355X, 1024 live streams, ms per push at 10 ms / 100 ms / 1 s chunks; C = push_device_io
 * (F32, F16) with the chunks at *_stream_input_ptr, B = the f32 push followed by a torch cast of the rows to f16 and a synchronise; D =
 * push_device_io (S16, F16), Bs = B with a torch int16 -> f32 conversion of the chunks in front).  Kaldi: C 0.0537 / 0.0611 / 0.1381, B
 * 0.0679 / 0.0755 / 0.1547, D 0.0662 / 0.0736 / 0.1629, Bs 0.0835 / 0.0908 / 0.1998.  NeMo f64: C 0.0557 / 0.0640 / 0.1437, B 0.0699 /
 * 0.0770 / 0.1673, D 0.0695 / 0.0779 / 0.1677, Bs 0.0857 / 0.0948 / 0.2133.  NeMo MELSPEC_PRECISION_F32: C 0.0565 / 0.0605 / 0.1269, B
 * 0.0704 / 0.0728 / 0.1521, D 0.0702 / 0.0729 / 0.1512, Bs 0.0859 / 0.0893 / 0.1912.  C and D are faster than B and Bs at every size
 * (0.79 - 0.89 x); the typed push costs 0.97 - 1.07 x of the f32 push. */
int melspec_fbank_stream_supports_io(const void *st, int pcm_dtype, int out_dtype);
int melspec_fbank_stream_push_host_io(void *st, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n,
                                      void *out, int out_dtype, size_t out_capacity_elems, uint32_t *frames_out);
int melspec_fbank_stream_push_device_io(void *st, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets,
                                        const uint32_t *lens, uint32_t n, void *d_out, int out_dtype, const uint64_t *h_out_offsets,
                                        uint32_t *frames_out, void *stream);

int melspec_blm_stream_supports_io(const void *st, int pcm_dtype, int out_dtype);
int melspec_blm_stream_push_host_io(void *st, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n,
                                    void *out, int out_dtype, size_t out_capacity_elems, uint32_t *frames_out);
int melspec_blm_stream_push_device_io(void *st, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets,
                                      const uint32_t *lens, uint32_t n, void *d_out, int out_dtype, const uint64_t *h_out_offsets,
                                      uint32_t *frames_out, void *stream);
int melspec_blm_stream_finish_host_io(void *st, const uint32_t *ids, uint32_t n, void *out, int out_dtype, size_t out_capacity_elems,
                                      uint32_t *frames_out);
int melspec_blm_stream_finish_device_io(void *st, const uint32_t *ids, uint32_t n, void *d_out, int out_dtype,
                                        const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream);

/* ---- 8-bit quantisation + TGA container: replaces src/quant.rs ------------------------ */
/* The reference's wire/disk format right after the mel path: a mel-major interleaved image
 * ([n_mels][width] f32, what melspec_compute_uniform_device_interleaved(.., major_column_order = 0, ..)
 * writes) is quantised to u8 with its own {min,max} and wrapped in an 18-byte TARGA header plus an 8-byte
 * ID field holding {min,max} as little-endian f32 (tga_8bit_data, src/quant.rs:38-64).  Bytes are
 * identical to the CPU's: the arithmetic is the reference's f32 sequence (quantize, src/quant.rs:140-153:
 * f32::min/max folds that skip NaN, scale = 255/(max-min), round half away from zero, clamp). */
typedef struct melspec_tga melspec_tga;

int melspec_tga_create(melspec_tga **out, int device);
void melspec_tga_destroy(melspec_tga *q);

/* tga_8bit (src/quant.rs:29-36) cuts an image into chunks of <= 65535 columns
 * (chunk_frames_into_strides, :100-136), one TGA each.  Layout used by this library for the
 * Vec<Vec<u8>> it returns: chunk c of an image starts at byte c * chunk_stride (a multiple of 4);
 * every chunk but the last holds 26 + n_mels*65535 bytes, the last one last_chunk_bytes.
 * width == 0 -> 0 chunks. */
int melspec_tga_layout(int n_mels, size_t width, uint32_t *n_chunks, size_t *chunk_stride, size_t *last_chunk_bytes);

/* n_images images, image i at d_images + i*image_stride floats -> blobs at d_blobs + i*blob_stride bytes
 * (blob_stride a multiple of 4, >= n_chunks*chunk_stride; d_blobs 4-byte aligned).  Asynchronous on
 * `stream` (NULL -> the handle's stream).  save_tga_8bit (src/quant.rs:15-27) is this plus a file write. */
int melspec_tga_encode_device(melspec_tga *q, const float *d_images, size_t image_stride, int n_mels, size_t width,
                              uint32_t n_images, uint8_t *d_blobs, size_t blob_stride, void *stream);
/* parse_tga_8bit / load_tga_8bit (src/quant.rs:66-98) for the same layout: reads {min,max} from bytes
 * 18..25 of every chunk and dequantises (dequantize, :156-165: u8 * ((max-min)/255) + min, two roundings). */
/* PCM -> TGA blobs, device resident: tga_8bit_data(interleave_frames(mel(clip), false, min_width)) for n_clips uniform clips
 * (src/quant.rs:38-64, src/mel.rs:480-544), the images left in d_images ([n_clips][n_mels][W], W = melspec_interleaved_width) and one
 * blob per clip at d_blobs + i * blob_stride (melspec_tga_layout).  On the fused n_fft = 400 kernels the mel kernel folds each image's
 * {min, max} while it stores it, so the quantiser reads the image once: same bytes as melspec_compute_uniform_device_interleaved followed
 * by melspec_tga_encode_device.  `q` and `ctx` must be on one device; asynchronous on `stream` (NULL: the context's). */
int melspec_tga_encode_pcm_uniform_device(melspec_tga *q, melspec_ctx *ctx, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                          uint32_t n_clips, uint64_t min_width, float *d_images, uint8_t *d_blobs, size_t blob_stride,
                                          void *stream);
int melspec_tga_decode_device(melspec_tga *q, const uint8_t *d_blobs, size_t blob_stride, int n_mels, size_t width,
                              uint32_t n_images, float *d_images, size_t image_stride, void *stream);
/* tga_8bit(data, n_mels) on host memory; n_chunks blobs laid out as melspec_tga_layout says. */
int melspec_tga_encode_host(melspec_tga *q, const float *data, size_t len, int n_mels, uint8_t *out, size_t out_capacity,
                            uint32_t *n_chunks);
/* parse_tga_8bit(blob): skips the 18 header bytes without looking at them, like the reference;
 * n_bytes < 26 -> MELSPEC_ERR_INVALID_ARG ("failed to fill whole buffer"). */
int melspec_tga_decode_host(melspec_tga *q, const uint8_t *blob, size_t n_bytes, float *out, size_t out_capacity, size_t *n_values);

/* quantize / dequantize without the container (src/quant.rs:140-165; src/wasm.rs:113 uses it per frame).
 * range = {min, max}.  Device variants: d_out needs n rounded up to a multiple of 4 bytes. */
int melspec_quantize_device(melspec_tga *q, const float *d_frame, size_t n, uint8_t *d_out, float *d_range, void *stream);
int melspec_dequantize_device(melspec_tga *q, const uint8_t *d_data, size_t n, const float *d_range, float *d_out, void *stream);
int melspec_quantize_host(melspec_tga *q, const float *frame, size_t n, uint8_t *out, float *range);
int melspec_dequantize_host(melspec_tga *q, const uint8_t *data, size_t n, const float *range, float *out);
int melspec_tga_synchronize(melspec_tga *q);

/* ---- VAD column classification: vad_boundaries (src/vad.rs:256-340) -------------------- */
/* The reference's consumer of the mel image ([n_mels][width], what interleave_frames(.., false, ..) or
 * to_array2 (src/quant.rs:168-174) produce): a 3x3 Sobel stencil, per column the count of rows
 * y in [min(min_mel, n_mels-2), n_mels-2) whose squared gradient reaches min_energy^2, raw[x] = count >= min_y
 * (classify_columns_in_frame, :373-415), then a +-4 moving-window majority vote (smooth_mask, :343-360).
 * EdgeInfo::intersected() are the set entries of `smoothed`, non_intersected() the clear ones.  Same f64
 * arithmetic on the same f32 pixels as the reference: the masks are identical, not close. */
typedef struct melspec_vad_settings {      /* DetectionSettings, src/vad.rs:5-22 */
    double min_energy;                     /* 0.98 */
    int min_y;                             /* 11 */
    int min_x;                             /* 5: window of VoiceActivityDetector::add, not used by vad_boundaries */
    int min_mel;                           /* 2 */
} melspec_vad_settings;
void melspec_vad_default_settings(melspec_vad_settings *s);
/* width - 2, or 0 when n_mels < 3 or width < 3 (the reference then returns an empty EdgeInfo) */
size_t melspec_vad_mask_len(int n_mels, size_t width);
/* n_images images at d_images + i*image_stride floats -> byte masks at d_raw / d_smoothed + i*mask_stride
 * (melspec_vad_mask_len entries each) and, if d_longest_run != NULL, the longest run of consecutive intersected
 * columns per image (vad_on(edge_info, n), src/vad.rs:229-254, is `longest_run >= n` for n >= 2).
 * Asynchronous on `stream` of the current device. */
int melspec_vad_boundaries_device(const float *d_images, size_t image_stride, int n_mels, size_t width, uint32_t n_images,
                                  const melspec_vad_settings *settings, uint8_t *d_raw, uint8_t *d_smoothed, size_t mask_stride,
                                  uint32_t *d_longest_run, void *stream);
/* one image in host memory (device < 0: the current one); raw_out may be NULL */
int melspec_vad_boundaries_host(int device, const float *image, int n_mels, size_t width, const melspec_vad_settings *settings,
                                uint8_t *raw_out, uint8_t *smoothed_out, uint32_t *longest_run);

/* ---- the detector inside the streaming bank: VoiceActivityDetector::{new, add, add_activity}, src/vad.rs:137-208, per stream ----
 * The reference keeps the last min_x mel frames of a stream and runs vad_boundaries on that [n_mels][min_x] window for every frame
 * it is given.  With the stage on, every push / flush of the bank also feeds its streams' detectors on the device, from the mel rows
 * the push has just written (no copy back, no launch per frame): each frame costs one 3-column Sobel walk, the stream's state is its
 * last two rows and 64 bits of column history in HBM.  One record per emitted frame, packed in entry order like the rows:
 *   valid = 0 where add_activity returns None (fewer than min_x frames so far); otherwise active, leading_active_columns,
 *   active_columns and window_columns are VoiceActivity's fields (confidence = active_columns / window_columns or 0,
 *   frame_index = melspec_stream_vad_frames before the push + the frame's position in it).
 * Decisions are made on the f32 mel rows the path stores, widened to f64 like the reference's arithmetic.  settings == NULL turns the
 * stage off; turning it on (or melspec_stream_reset) starts every (listed) detector afresh.  min_x <= 66. */
typedef struct melspec_vad_activity {
    uint8_t valid, active;
    uint16_t leading_active_columns, active_columns, window_columns;
} melspec_vad_activity;
int melspec_stream_enable_vad(melspec_stream *st, const melspec_vad_settings *settings);
/* frames stream id has fed to its detector (the frame_index of the next one) */
uint64_t melspec_stream_vad_frames(const melspec_stream *st, uint32_t id);
/* melspec_stream_push_host / _flush_host / _push_device that also return the records (acts: host memory for the host calls, device
 * memory for the device call; capacity in records >= the frames the call emits) */
int melspec_stream_push_host_vad(melspec_stream *st, const uint32_t *ids, const float *samples, const uint32_t *lens, uint32_t n,
                                 float *out, size_t out_capacity_floats, uint32_t *frames_out, melspec_vad_activity *acts,
                                 size_t acts_capacity);
int melspec_stream_flush_host_vad(melspec_stream *st, const uint32_t *ids, uint32_t n, float *out, size_t out_capacity_floats,
                                  uint32_t *frames_out, melspec_vad_activity *acts, size_t acts_capacity);
int melspec_stream_push_device_vad(melspec_stream *st, const uint32_t *ids, const uint32_t *lens, uint32_t n, float *d_out,
                                   const uint64_t *out_offsets, uint32_t *frames_out, melspec_vad_activity *d_acts, void *stream);

/* ---- device memory helpers for hosts with no HIP binding of their own --------------- */
/* (what the cudaMalloc/cudaMemcpyAsync externs of src/cuda.rs:185-199 give the Rust side) */
int melspec_malloc(void **dptr, size_t bytes);
int melspec_free(void *dptr);
int melspec_memcpy_h2d(void *dst_device, const void *src_host, size_t bytes);
int melspec_memcpy_d2h(void *dst_host, const void *src_device, size_t bytes);
int melspec_device_synchronize(void);

/* Synthetic PCM of SURVEY.md §8(d), generated on the device for benches/tests:
 * d_out[c*clip_stride + i] = hashnoise(seed, first_clip + c, i), c < n_clips, i < clip_len. */
int melspec_synth_pcm_device(float *d_out, uint64_t clip_stride, uint64_t clip_len,
                             uint64_t first_clip, uint32_t n_clips, uint32_t seed, void *stream);
/* samples [first_sample, first_sample + n_samples) of the same clips (a live producer for the streaming bank) */
int melspec_synth_pcm_window_device(float *d_out, uint64_t clip_stride, uint64_t first_sample, uint64_t n_samples,
                                    uint64_t first_clip, uint32_t n_clips, uint32_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MELSPEC_HIP_H */
