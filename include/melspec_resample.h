/* melspec_resample.h -- the stage in front of the frontends: PCM at 8-96 kHz, int16 or f32, resampled on the GPU to f32 PCM at the
 * model rate, in device memory, ready for the melspec_* device calls on the same stream.  A polyphase windowed-sinc filter, new gfx950
 * HIP (mel_spec_amd/csrc/resample.hip).  A header of its own: the opaque handle below is not one of melspec_hip.h's types.  It uses
 * that header's status codes and MELSPEC_PCM_* codes; melspec_abi_version() stays 1.
 *
 * THE DEFINITION.  The filter is torchaudio.functional.resample's default: sinc_interp_hann, lowpass_filter_width = 6, rolloff = 0.99,
 * written with integer arguments so that every implementation gets the same taps.  For rate_in, rate_out >= 1:
 *   g = gcd(rate_in, rate_out), orig = rate_in / g, new = rate_out / g, M = max(orig, new), m_ = min(orig, new)
 *   width = ceil(600 orig / (99 m_)) in integer arithmetic,  K = 2 width + orig
 * For phase p in [0, new) and tap k in [0, K):
 *   m = (k - width) new - p orig, an integer
 *   the tap is INSIDE iff 99 |m| < 600 M; outside taps are exactly 0 (torchaudio's clamped ends are about 4e-33 there: the only deviation)
 *   t = (99.0 m) / (100.0 M) in f64
 *   h[p][k] = sinc(pi t) cos^2(pi t / 12) (99.0 m_) / (100.0 orig),  sinc(0) = 1
 * The inside taps of a phase are contiguous.  For a clip x of L samples, zero outside [0, L):
 *   out_len = ceil(new L / orig);  for i = j new + p < out_len:  y[i] = sum_k h[p][k] x[j orig + k - width]
 * An int16 sample has the value s * 2^-15 exactly.  Products and sums are f64 with the f64 taps and are rounded to f32 once, at the store.
 * rate_in == rate_out is a plain exact copy (int16 -> f32 conversion), no filter.
 * The kernel multiplies, per output, the max_inside_taps taps of a window that holds the phase's inside taps and lies inside [0, K): a
 * non-finite sample makes the outputs non-finite whose inside taps reach it, and may do so for outputs whose dense window
 * [j orig - width, j orig + width + orig) holds it; every other output is untouched by it.
 *
 * CONVENTIONS, those of the _io calls of melspec_hip.h.  Strides, offsets and lengths count ELEMENTS.  Only natural alignment of the
 * element type is required: a ragged int16 clip may start at an odd sample.  Device calls are stream-ordered and asynchronous (stream:
 * a hipStream_t, NULL = the resampler's own stream); the host tables are read before the call returns; the host call is synchronous.  A
 * refused call queues nothing and writes nothing.  n_clips == 0 and zero-length clips are MELSPEC_OK.  Nothing at or past a clip's out_len
 * is written.  All index arithmetic on samples is 64-bit.
 * Statuses, in this order: a NULL handle; an unknown dtype code; NULL pointers (of a call with samples to read); pointers that are not
 * aligned to their element type; out_stride < out_len -- all MELSPEC_ERR_INVALID_ARG.  A zero rate is MELSPEC_ERR_INVALID_ARG; a
 * reduced orig or new above 4096 is MELSPEC_ERR_UNSUPPORTED; no usable device is MELSPEC_ERR_UNAVAILABLE; a too-small capacity is
 * MELSPEC_ERR_CAPACITY.  One resampler per thread and device, as the other objects.
 *
 * OUT OF SCOPE here: a clip table in device memory (_desc); a streaming resampler with carried history; 16-bit output; other filter
 * widths or rolloffs; the sharded object. */
#ifndef MELSPEC_RESAMPLE_H
#define MELSPEC_RESAMPLE_H

#include "melspec_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct melspec_resampler melspec_resampler;

/* ---- no device needed ---- */
/* The geometry of a rate pair; any of the four pointers may be NULL. */
int melspec_resample_geometry(uint32_t rate_in, uint32_t rate_out, uint32_t *orig, uint32_t *new_rate, uint32_t *width, uint32_t *max_inside_taps);
/* The dense tap table, taps[p * K + k]; capacity in doubles, at least new * K. */
int melspec_resample_taps(uint32_t rate_in, uint32_t rate_out, double *taps, size_t capacity);
/* ceil(new n_in / orig); 0 for a zero rate. */
size_t melspec_resample_out_len(uint32_t rate_in, uint32_t rate_out, size_t n_in);

/* ---- the object ---- */
/* device < 0: the current device.  The arguments are checked before a device is looked for. */
int melspec_resampler_create(melspec_resampler **out, int device, uint32_t rate_in, uint32_t rate_out);
void melspec_resampler_destroy(melspec_resampler *r);
/* Which form of the kernel this rate pair runs on (samples and taps in LDS for every usual rate). */
const char *melspec_resampler_kernel_name(const melspec_resampler *r);
/* n_clips clips of clip_len samples, clip i at d_pcm + i * clip_stride, its out_len outputs at d_out + i * out_stride. */
int melspec_resample_uniform_device(melspec_resampler *r, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips, float *d_out, uint64_t out_stride, void *stream);
/* Clip i is h_lengths[i] samples at d_pcm + h_offsets[i]; its outputs go to d_out + h_out_offsets[i] (NULL: packed in clip order). */
int melspec_resample_ragged_device(melspec_resampler *r, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips, float *d_out, const uint64_t *h_out_offsets, void *stream);
/* One clip from host memory to host memory; *n_out (may be NULL) = out_len on success. */
int melspec_resample_host(melspec_resampler *r, const void *samples, int pcm_dtype, size_t n_samples, float *out, size_t out_capacity, size_t *n_out);
int melspec_resampler_synchronize(melspec_resampler *r, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MELSPEC_RESAMPLE_H */
