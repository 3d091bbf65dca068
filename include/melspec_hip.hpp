// melspec_hip.hpp -- header-only C++ host mirror of the reference's plugin interface, over the C ABI
// (melspec_hip.h).  Same names, argument order and error split as the reference's Rust types:
//
//   melspec::HipMelSpectrogram(fft_size, hop_size, sampling_rate, n_mels)   CudaMelSpectrogram::new   src/cuda.rs:39-82
//   .compute_mel_spectrogram(samples) -> vector<vector<float>>              src/cuda.rs:88-101
//   melspec::Fbank(FbankConfig{}).compute(samples) -> Array2f               Fbank::{new,compute}      src/fbank.rs:94,141
//   melspec::mel(sr, n_fft, n_mels, f_min, f_max, htk, norm)                mel()                     src/mel.rs:547-589
//
// HipUnavailable == CudaError::Unavailable (construction; callers may skip), HipRuntimeError ==
// CudaError::Runtime (per call).  Objects are move-only and single-threaded, like `&mut self`.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "melspec_hip.h"

namespace melspec {

struct HipError : std::runtime_error {
    int code;
    HipError(int c, const std::string &m) : std::runtime_error("[" + std::to_string(c) + "] " + m), code(c) {}
};
struct HipUnavailable : HipError { using HipError::HipError; };
struct HipRuntimeError : HipError { using HipError::HipError; };

namespace detail {
inline void check(int rc, bool constructing) {
    if (rc == MELSPEC_OK) return;
    const char *m = melspec_last_error();
    if (constructing || rc == MELSPEC_ERR_UNAVAILABLE) throw HipUnavailable(rc, m ? m : "");
    throw HipRuntimeError(rc, m ? m : "");
}
}  // namespace detail

class HipMelSpectrogram {
public:
    HipMelSpectrogram(std::size_t fft_size, std::size_t hop_size, double sampling_rate, std::size_t n_mels, int device = -1) {
        detail::check(melspec_create(&ctx_, device, static_cast<int>(fft_size), static_cast<int>(hop_size), sampling_rate,
                                     static_cast<int>(n_mels)), true);
    }
    // MelSpectrogram over SparseMelFilterbank::from_mel(sr, n_fft, n_mels, f_min, f_max, htk, norm) (src/mel.rs:73-87); f_min < 0 / f_max <= 0 == None
    static HipMelSpectrogram with_filterbank(std::size_t fft_size, std::size_t hop_size, double sampling_rate, std::size_t n_mels, double f_min,
                                             double f_max, bool htk, bool norm, int device = -1) {
        HipMelSpectrogram m;
        detail::check(melspec_create_with_filterbank(&m.ctx_, device, static_cast<int>(fft_size), static_cast<int>(hop_size), sampling_rate,
                                                     static_cast<int>(n_mels), f_min, f_max, htk ? 1 : 0, norm ? 1 : 0), true);
        return m;
    }
    // ... over SparseMelFilterbank::from_dense (src/mel.rs:48-71): filters = [n_mels][fft_size / 2 + 1], row-major
    static HipMelSpectrogram with_dense_filterbank(std::size_t fft_size, std::size_t hop_size, double sampling_rate, std::size_t n_mels,
                                                   const std::vector<double> &filters, int device = -1) {
        HipMelSpectrogram m;
        detail::check(melspec_create_with_dense_filterbank(&m.ctx_, device, static_cast<int>(fft_size), static_cast<int>(hop_size), sampling_rate,
                                                           static_cast<int>(n_mels), filters.data(), static_cast<int>(filters.size() / (n_mels ? n_mels : 1))), true);
        return m;
    }
    ~HipMelSpectrogram() { melspec_destroy(ctx_); }
    HipMelSpectrogram(HipMelSpectrogram &&o) noexcept : ctx_(std::exchange(o.ctx_, nullptr)) {}
    HipMelSpectrogram &operator=(HipMelSpectrogram &&o) noexcept {
        if (this != &o) { melspec_destroy(ctx_); ctx_ = std::exchange(o.ctx_, nullptr); }
        return *this;
    }
    HipMelSpectrogram(const HipMelSpectrogram &) = delete;
    HipMelSpectrogram &operator=(const HipMelSpectrogram &) = delete;

    std::size_t n_mels() const { return static_cast<std::size_t>(melspec_n_mels(ctx_)); }
    std::size_t num_frames(std::size_t n_samples) const { return melspec_num_frames(ctx_, n_samples); }

    // frames x n_mels, row-major, one inner vector per frame like the reference's Vec<Vec<f32>>
    std::vector<std::vector<float>> compute_mel_spectrogram(const std::vector<float> &samples) {
        const std::size_t frames = num_frames(samples.size()), nm = n_mels();
        std::vector<float> flat(frames * nm);
        std::size_t got = 0;
        detail::check(melspec_compute_host(ctx_, samples.data(), samples.size(), flat.data(), flat.size(), &got), false);
        std::vector<std::vector<float>> out(got);
        for (std::size_t f = 0; f < got; ++f) out[f].assign(flat.begin() + f * nm, flat.begin() + (f + 1) * nm);
        return out;
    }

    // device-resident batch of equal-length clips (additive surface)
    void compute_uniform_device(const float *d_pcm, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips,
                                float *d_out, void *stream = nullptr) {
        detail::check(melspec_compute_uniform_device(ctx_, d_pcm, clip_stride, clip_len, n_clips, d_out, stream), false);
    }
    void synchronize(void *stream = nullptr) { detail::check(melspec_synchronize(ctx_, stream), false); }
    // f64 window/FFT/power like the reference's CPU and CUDA paths (melspec_set_precise)
    void set_precise(bool on) { detail::check(melspec_set_precise(ctx_, on ? 1 : 0), false); }
    bool precise() const { return melspec_is_precise(ctx_) != 0; }
    // MELSPEC_PRECISION_AUTO (default) / _F64 / _F32
    void set_precision(int mode) { detail::check(melspec_set_precision(ctx_, mode), false); }
    int precision() const { return melspec_precision(ctx_); }
    // AUTO moves whole batches to the f64 kernel while most frames of the last finished batch needed f64; false pins the f32 kernel
    void set_auto_adaptive(bool on) { detail::check(melspec_set_auto_adaptive(ctx_, on ? 1 : 0), false); }
    bool auto_heavy() { int h = 0; double f = 0.0; detail::check(melspec_auto_state(ctx_, &h, &f), false); return h != 0; }
    // CudaMelSpectrogram::max_frames_per_batch (src/cuda.rs:84-86): frames per chunk of the host pipeline
    std::size_t max_frames_per_batch() const { return melspec_max_frames_per_batch(ctx_); }

    // additive: many host clips in one call through the chunked H2D / kernels / D2H pipeline -> [clip][frame][mel]
    std::vector<std::vector<std::vector<float>>> compute_batch(const std::vector<std::vector<float>> &clips) {
        std::vector<std::uint64_t> offs, lens;
        std::vector<float> flat;
        for (const auto &c : clips) { offs.push_back(flat.size()); lens.push_back(c.size()); flat.insert(flat.end(), c.begin(), c.end()); }
        const std::size_t nm = n_mels();
        std::size_t total = 0;
        for (const auto &c : clips) total += num_frames(c.size());
        std::vector<float> out(total * nm + 1);
        std::uint64_t got = 0;
        if (flat.empty()) flat.push_back(0.0f);
        detail::check(melspec_compute_batch_host(ctx_, flat.data(), offs.data(), lens.data(), static_cast<std::uint32_t>(clips.size()),
                                                 out.data(), nullptr, out.size(), &got), false);
        std::vector<std::vector<std::vector<float>>> res(clips.size());
        std::size_t cur = 0;
        for (std::size_t c = 0; c < clips.size(); ++c) {
            const std::size_t f = num_frames(clips[c].size());
            res[c].resize(f);
            for (std::size_t i = 0; i < f; ++i, cur += nm) res[c][i].assign(out.begin() + cur, out.begin() + cur + nm);
        }
        return res;
    }

    // Spectrogram::compute_all_cpu (src/stft.rs:89-115): [frame][fft_size] interleaved (re, im) doubles
    std::vector<std::vector<double>> compute_all(const std::vector<float> &samples) {
        const std::size_t frames = num_frames(samples.size()), bins = melspec_stft_bins(ctx_, 1);
        std::vector<double> flat(frames * bins * 2 + 2);
        std::size_t got = 0;
        detail::check(melspec_stft_host(ctx_, samples.data(), samples.size(), flat.data(), frames * bins, MELSPEC_STFT_F64, 1, &got), false);
        std::vector<std::vector<double>> out(got);
        for (std::size_t f = 0; f < got; ++f) out[f].assign(flat.begin() + f * bins * 2, flat.begin() + (f + 1) * bins * 2);
        return out;
    }
    // MelSpectrogram::add(&fft) (src/mel.rs:13-32) for every frame of compute_all's output (or any [frame][fft_size] (re, im) doubles)
    std::vector<std::vector<float>> mel_from_stft(const std::vector<std::vector<double>> &frames) {
        const std::size_t nm = static_cast<std::size_t>(melspec_n_mels(ctx_)), bins = melspec_stft_bins(ctx_, 1);
        std::vector<double> flat;
        flat.reserve(frames.size() * bins * 2);
        for (const auto &f : frames) flat.insert(flat.end(), f.begin(), f.end());
        std::vector<float> out(frames.size() * nm + 1);
        detail::check(melspec_mel_from_stft_host(ctx_, flat.data(), MELSPEC_STFT_F64, 1, frames.size(), out.data(), out.size()), false);
        std::vector<std::vector<float>> res(frames.size());
        for (std::size_t f = 0; f < frames.size(); ++f) res[f].assign(out.begin() + f * nm, out.begin() + (f + 1) * nm);
        return res;
    }
    // ---- Whisper features as the encoders were trained on them (melspec_whisper_*: centred STFT, pad / trim to pad_to, clip-wide clamp) ----
    bool supports_whisper() const { return melspec_whisper_supports(ctx_) != 0; }
    std::size_t whisper_num_frames(std::size_t n_samples, std::size_t pad_to = 480000) const { return melspec_whisper_num_frames(ctx_, n_samples, pad_to); }
    const char *whisper_kernel_name() const { return melspec_whisper_kernel_name(ctx_); }
    // one host clip -> [n_mels][T] (mel_major: what the encoders take) or [T][n_mels], flat
    std::vector<float> whisper_features(const std::vector<float> &samples, std::size_t pad_to = 480000, bool mel_major = true, std::size_t *n_frames = nullptr) {
        const std::size_t T = whisper_num_frames(samples.size(), pad_to);
        std::vector<float> out(T * static_cast<std::size_t>(melspec_n_mels(ctx_)) + 1);
        std::size_t nf = 0;
        detail::check(melspec_whisper_compute_host(ctx_, samples.data(), samples.size(), pad_to, out.data(), out.size(), mel_major ? 1 : 0, &nf), false);
        out.resize(nf * static_cast<std::size_t>(melspec_n_mels(ctx_)));
        if (n_frames) *n_frames = nf;
        return out;
    }
    // device pointers in and out, asynchronous on `stream` (nullptr: the context's)
    void whisper_uniform_device(const float *d_pcm, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, std::uint64_t pad_to, float *d_out,
                                bool mel_major = true, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_uniform_device(ctx_, d_pcm, clip_stride, clip_len, n_clips, pad_to, d_out, mel_major ? 1 : 0, stream), false);
    }
    void whisper_ragged_device(const float *d_pcm, const std::vector<std::uint64_t> &offsets, const std::vector<std::uint64_t> &lengths, std::uint64_t pad_to,
                               float *d_out, const std::uint64_t *out_offsets = nullptr, bool mel_major = true, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_ragged_device(ctx_, d_pcm, offsets.data(), lengths.data(), static_cast<std::uint32_t>(offsets.size()), pad_to, d_out,
                                                            out_offsets, mel_major ? 1 : 0, stream), false);
    }
    // split output: raw log10 rows [T][n_mels] per clip + the clips' maxima; the consumer folds (max(x, g - 8) + 4) / 4 into its first read
    void whisper_uniform_device_split(const float *d_pcm, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, std::uint64_t pad_to,
                                      float *d_rows, float *d_clip_max, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_uniform_device_split(ctx_, d_pcm, clip_stride, clip_len, n_clips, pad_to, d_rows, d_clip_max, stream), false);
    }
    void whisper_ragged_device_split(const float *d_pcm, const std::vector<std::uint64_t> &offsets, const std::vector<std::uint64_t> &lengths, std::uint64_t pad_to,
                                     float *d_rows, float *d_clip_max, const std::uint64_t *rows_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_ragged_device_split(ctx_, d_pcm, offsets.data(), lengths.data(), static_cast<std::uint32_t>(offsets.size()), pad_to,
                                                                  d_rows, rows_offsets, d_clip_max, stream), false);
    }
    // the ragged calls with their clip table in device memory (melspec_whisper_compute_ragged_device_desc*): u64 offsets / lengths / output offsets
    // read by a planner kernel on `stream`; pad_to >= 400; the bits of the host-table calls.  The _io forms take MELSPEC_PCM_* / MELSPEC_OUT_*.
    bool supports_whisper_desc() const { return melspec_whisper_supports_desc(ctx_) != 0; }
    void whisper_ragged_device_desc(const float *d_pcm, const std::uint64_t *d_offsets, const std::uint64_t *d_lengths, std::uint32_t n_clips, float *d_out,
                                    std::uint64_t pad_to = 480000, const std::uint64_t *d_out_offsets = nullptr, bool mel_major = true, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_ragged_device_desc(ctx_, d_pcm, d_offsets, d_lengths, n_clips, pad_to, d_out, d_out_offsets, mel_major ? 1 : 0, stream), false);
    }
    void whisper_ragged_device_desc_split(const float *d_pcm, const std::uint64_t *d_offsets, const std::uint64_t *d_lengths, std::uint32_t n_clips, float *d_rows,
                                          float *d_clip_max, std::uint64_t pad_to = 480000, const std::uint64_t *d_rows_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_ragged_device_desc_split(ctx_, d_pcm, d_offsets, d_lengths, n_clips, pad_to, d_rows, d_rows_offsets, d_clip_max, stream), false);
    }
    void whisper_ragged_device_desc_io(const void *d_pcm, int pcm_dtype, const std::uint64_t *d_offsets, const std::uint64_t *d_lengths, std::uint32_t n_clips,
                                       void *d_out, int out_dtype, std::uint64_t pad_to = 480000, const std::uint64_t *d_out_offsets = nullptr, bool mel_major = true,
                                       void *stream = nullptr) {
        detail::check(melspec_whisper_compute_ragged_device_desc_io(ctx_, d_pcm, pcm_dtype, d_offsets, d_lengths, n_clips, pad_to, d_out, out_dtype, d_out_offsets,
                                                                    mel_major ? 1 : 0, stream), false);
    }
    void whisper_ragged_device_desc_split_io(const void *d_pcm, int pcm_dtype, const std::uint64_t *d_offsets, const std::uint64_t *d_lengths, std::uint32_t n_clips,
                                             void *d_rows, int out_dtype, float *d_clip_max, std::uint64_t pad_to = 480000,
                                             const std::uint64_t *d_rows_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_whisper_compute_ragged_device_desc_split_io(ctx_, d_pcm, pcm_dtype, d_offsets, d_lengths, n_clips, pad_to, d_rows, out_dtype, d_rows_offsets,
                                                                          d_clip_max, stream), false);
    }
    melspec_ctx *raw() { return ctx_; }

private:
    HipMelSpectrogram() = default;          // the factories above
    melspec_ctx *ctx_ = nullptr;
};

struct FbankConfig : melspec_fbank_config {
    FbankConfig() { melspec_fbank_default_config(this); }   // FbankConfig::default, src/fbank.rs:46-64
};

struct Array2f {   // Array2<f32> (rows, cols), row-major
    std::size_t rows = 0, cols = 0;
    std::vector<float> data;
    float operator()(std::size_t r, std::size_t c) const { return data[r * cols + c]; }
};

class Fbank {
public:
    explicit Fbank(const FbankConfig &cfg = FbankConfig(), int device = -1) {
        detail::check(melspec_fbank_create(&fb_, device, &cfg), true);
    }
    ~Fbank() { melspec_fbank_destroy(fb_); }
    Fbank(const Fbank &) = delete;
    Fbank &operator=(const Fbank &) = delete;

    Array2f compute(const std::vector<float> &samples) {
        Array2f a;
        a.cols = static_cast<std::size_t>(melspec_fbank_num_mel_bins(fb_));
        a.rows = melspec_fbank_num_frames(fb_, samples.size());
        a.data.assign(a.rows * a.cols, 0.0f);
        std::size_t got = 0;
        detail::check(melspec_fbank_compute_host(fb_, samples.data(), samples.size(), a.data.data(), a.data.size(), &got), false);
        return a;
    }

    // additive: compute() for many clips in one call (melspec_fbank_compute_batch_host)
    std::vector<Array2f> compute_batch(const std::vector<std::vector<float>> &clips) {
        std::vector<std::uint64_t> offs, lens;
        std::vector<float> flat;
        std::size_t total = 0;
        const std::size_t nm = static_cast<std::size_t>(melspec_fbank_num_mel_bins(fb_));
        for (const auto &c : clips) {
            offs.push_back(flat.size()); lens.push_back(c.size());
            flat.insert(flat.end(), c.begin(), c.end());
            total += melspec_fbank_num_frames(fb_, c.size());
        }
        std::vector<float> out(total * nm + 1);
        std::uint64_t frames = 0;
        detail::check(melspec_fbank_compute_batch_host(fb_, flat.data(), offs.data(), lens.data(), static_cast<std::uint32_t>(clips.size()),
                                                       out.data(), nullptr, out.size(), &frames), false);
        std::vector<Array2f> res(clips.size());
        std::size_t cur = 0;
        for (std::size_t i = 0; i < clips.size(); ++i) {
            res[i].rows = melspec_fbank_num_frames(fb_, clips[i].size());
            res[i].cols = nm;
            res[i].data.assign(out.begin() + cur, out.begin() + cur + res[i].rows * nm);
            cur += res[i].rows * nm;
        }
        return res;
    }

    // additive: 16-bit ends (MELSPEC_PCM_*, MELSPEC_OUT_* of melspec_hip.h); strides, offsets and lengths count elements
    bool supports_io(int pcm_dtype, int out_dtype) const { return melspec_fbank_supports_io(fb_, pcm_dtype, out_dtype) != 0; }
    void compute_uniform_device_io(const void *d_pcm, int pcm_dtype, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, void *d_out,
                                   int out_dtype, void *stream = nullptr) {
        detail::check(melspec_fbank_compute_uniform_device_io(fb_, d_pcm, pcm_dtype, clip_stride, clip_len, n_clips, d_out, out_dtype, stream), false);
    }
    void compute_ragged_device_io(const void *d_pcm, int pcm_dtype, const std::vector<std::uint64_t> &offsets, const std::vector<std::uint64_t> &lengths,
                                  void *d_out, int out_dtype, const std::uint64_t *out_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_fbank_compute_ragged_device_io(fb_, d_pcm, pcm_dtype, offsets.data(), lengths.data(), static_cast<std::uint32_t>(offsets.size()), d_out,
                                                             out_dtype, out_offsets, stream), false);
    }
    // compute() on 16-bit PCM (value = sample / 32768, exactly) into out_dtype features (MELSPEC_OUT_F16 / _BF16), returned as their bit
    // patterns, (frames, num_mel_bins) row-major: the int16 bytes are what crosses the bus
    std::vector<std::uint16_t> compute_s16(const std::vector<std::int16_t> &samples, int out_dtype, std::size_t *frames = nullptr) {
        std::vector<std::uint16_t> out(melspec_fbank_num_frames(fb_, samples.size()) * static_cast<std::size_t>(melspec_fbank_num_mel_bins(fb_)));
        std::size_t got = 0;
        detail::check(melspec_fbank_compute_host_io(fb_, samples.data(), MELSPEC_PCM_S16, samples.size(), out.data(), out_dtype, out.size(), &got), false);
        if (frames) *frames = got;
        return out;
    }
    // additive: the split output for ragged batches and with 16-bit ends (melspec_hip.h) -- the rows before CMN (16-bit rows: rounded
    // once) and the clips' f32 column means (the uniform f32 split's bits); strides, offsets and capacities count elements
    bool supports_split_io(int pcm_dtype, int out_dtype) const { return melspec_fbank_supports_split_io(fb_, pcm_dtype, out_dtype) != 0; }
    void compute_ragged_device_split(const float *d_pcm, const std::vector<std::uint64_t> &offsets, const std::vector<std::uint64_t> &lengths, float *d_rows,
                                     float *d_means, const std::uint64_t *rows_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_fbank_compute_ragged_device_split(fb_, d_pcm, offsets.data(), lengths.data(), static_cast<std::uint32_t>(offsets.size()), d_rows,
                                                                rows_offsets, d_means, stream), false);
    }
    void compute_uniform_device_split_io(const void *d_pcm, int pcm_dtype, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, void *d_rows,
                                         int out_dtype, float *d_means, void *stream = nullptr) {
        detail::check(melspec_fbank_compute_uniform_device_split_io(fb_, d_pcm, pcm_dtype, clip_stride, clip_len, n_clips, d_rows, out_dtype, d_means, stream), false);
    }
    void compute_ragged_device_split_io(const void *d_pcm, int pcm_dtype, const std::vector<std::uint64_t> &offsets, const std::vector<std::uint64_t> &lengths,
                                        void *d_rows, int out_dtype, float *d_means, const std::uint64_t *rows_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_fbank_compute_ragged_device_split_io(fb_, d_pcm, pcm_dtype, offsets.data(), lengths.data(), static_cast<std::uint32_t>(offsets.size()),
                                                                   d_rows, out_dtype, rows_offsets, d_means, stream), false);
    }
    struct SplitS16 {
        std::vector<std::uint16_t> rows;   // (frames, num_mel_bins) row-major, the bit patterns of out_dtype, before CMN
        std::size_t frames = 0;
        std::vector<float> means;          // (num_mel_bins)
    };
    SplitS16 compute_split_s16(const std::vector<std::int16_t> &samples, int out_dtype) {
        SplitS16 s;
        const std::size_t nm = static_cast<std::size_t>(melspec_fbank_num_mel_bins(fb_));
        s.rows.assign(melspec_fbank_num_frames(fb_, samples.size()) * nm, 0);
        s.means.assign(nm, 0.0f);
        detail::check(melspec_fbank_compute_host_split_io(fb_, samples.data(), MELSPEC_PCM_S16, samples.size(), s.rows.data(), out_dtype, s.rows.size(), s.means.data(),
                                                          &s.frames), false);
        return s;
    }
    // what the device calls above need from a class that does not hand out its handle: wait for a call that ran on the object's own
    // stream (stream == nullptr), and give back the scratch a 16-bit CMN call grows
    void synchronize(void *stream = nullptr) { detail::check(melspec_fbank_synchronize(fb_, stream), false); }
    void release_scratch() { detail::check(melspec_fbank_release_scratch(fb_), false); }

private:
    friend class FbankStreamBank;
    melspec_fbank *fb_ = nullptr;
};

// Fbank::compute fed chunk by chunk (melspec_fbank_stream_*): after pushes whose chunks concatenate to x a stream has emitted exactly the
// rows of compute(x) with apply_cmn off, before CMN whatever the object's setting; stats() gives the running column means of those rows.
// The Fbank must outlive the bank.
class FbankStreamBank {
public:
    FbankStreamBank(Fbank &fbank, std::size_t n_streams, std::size_t max_chunk) : n_mels_(static_cast<std::size_t>(melspec_fbank_num_mel_bins(fbank.fb_))) {
        detail::check(melspec_fbank_stream_create(&st_, fbank.fb_, static_cast<std::uint32_t>(n_streams), static_cast<std::uint32_t>(max_chunk)), true);
    }
    ~FbankStreamBank() { melspec_fbank_stream_destroy(st_); }
    FbankStreamBank(const FbankStreamBank &) = delete;
    FbankStreamBank &operator=(const FbankStreamBank &) = delete;

    void reset() { detail::check(melspec_fbank_stream_reset(st_, nullptr, 0), false); }
    void reset(const std::vector<std::uint32_t> &ids) { detail::check(melspec_fbank_stream_reset(st_, ids.data(), static_cast<std::uint32_t>(ids.size())), false); }
    std::size_t frames_after(std::uint32_t id, std::size_t n_new) const { return melspec_fbank_stream_frames_after(st_, id, static_cast<std::uint32_t>(n_new)); }
    // one chunk for one stream: the rows it completes, (frames, num_mel_bins) row-major
    Array2f push(std::uint32_t id, const std::vector<float> &chunk) { return push_typed(id, chunk.data(), MELSPEC_PCM_F32, chunk.size()); }
    Array2f push(std::uint32_t id, const std::vector<std::int16_t> &chunk) { return push_typed(id, chunk.data(), MELSPEC_PCM_S16, chunk.size()); }
    float *input_ptr(std::uint32_t id) { return melspec_fbank_stream_input_ptr(st_, id); }
    void push_device(const std::vector<std::uint32_t> &ids, const void *d_chunks, int pcm_dtype, const std::uint64_t *src_offsets, const std::vector<std::uint32_t> &lens,
                     float *d_out, const std::uint64_t *out_offsets, std::uint32_t *frames_out, void *stream = nullptr) {
        detail::check(melspec_fbank_stream_push_device(st_, ids.data(), d_chunks, pcm_dtype, src_offsets, lens.data(), static_cast<std::uint32_t>(ids.size()), d_out,
                                                       out_offsets, frames_out, stream), false);
    }
    // mean[bin] = float(f64 sum of the stream's rows / count); count = rows emitted so far
    std::vector<float> stats(std::uint32_t id, std::uint64_t *count = nullptr) {
        std::vector<float> means(n_mels_);
        detail::check(melspec_fbank_stream_stats_host(st_, &id, 1, means.data(), count), false);
        return means;
    }
    void stats_device(const std::vector<std::uint32_t> &ids, float *d_means, std::uint64_t *counts, void *stream = nullptr) {
        detail::check(melspec_fbank_stream_stats_device(st_, ids.data(), static_cast<std::uint32_t>(ids.size()), d_means, counts, stream), false);
    }

    // additive: f16 / bf16 rows out (MELSPEC_OUT_* of melspec_hip.h); offsets count elements of the row type, stats() stays that of the f32 rows
    bool supports_io(int pcm_dtype, int out_dtype) const { return melspec_fbank_stream_supports_io(st_, pcm_dtype, out_dtype) != 0; }
    // push() on 16-bit PCM into out_dtype rows (MELSPEC_OUT_F16 / _BF16), returned as their bit patterns, (frames, num_mel_bins) row-major
    std::vector<std::uint16_t> push_s16(std::uint32_t id, const std::vector<std::int16_t> &chunk, int out_dtype, std::size_t *frames = nullptr) {
        std::vector<std::uint16_t> out(frames_after(id, chunk.size()) * n_mels_);
        const std::uint32_t len = static_cast<std::uint32_t>(chunk.size());
        std::uint32_t got = 0;
        detail::check(melspec_fbank_stream_push_host_io(st_, &id, chunk.data(), MELSPEC_PCM_S16, &len, 1, out.data(), out_dtype, out.size(), &got), false);
        if (frames) *frames = got;
        return out;
    }
    void push_device_io(const std::vector<std::uint32_t> &ids, const void *d_chunks, int pcm_dtype, const std::uint64_t *src_offsets,
                        const std::vector<std::uint32_t> &lens, void *d_out, int out_dtype, const std::uint64_t *out_offsets, std::uint32_t *frames_out,
                        void *stream = nullptr) {
        detail::check(melspec_fbank_stream_push_device_io(st_, ids.data(), d_chunks, pcm_dtype, src_offsets, lens.data(), static_cast<std::uint32_t>(ids.size()), d_out,
                                                          out_dtype, out_offsets, frames_out, stream), false);
    }

private:
    Array2f push_typed(std::uint32_t id, const void *samples, int pcm_dtype, std::size_t n) {
        Array2f a;
        const std::uint32_t len = static_cast<std::uint32_t>(n);
        a.cols = n_mels_;
        a.data.assign(frames_after(id, n) * n_mels_, 0.0f);
        std::uint32_t got = 0;
        detail::check(melspec_fbank_stream_push_host(st_, &id, samples, pcm_dtype, &len, 1, a.data.data(), a.data.size(), &got), false);
        a.rows = got;
        return a;
    }
    void *st_ = nullptr;
    std::size_t n_mels_;
};

struct BatchLogMelConfig : melspec_blm_config {
    BatchLogMelConfig() { melspec_blm_default_config(this); }   // BatchLogMelConfig::default, src/mel.rs:189-208
};

// BatchLogMelSpectrogram (src/mel.rs:239-396): the NeMo / Parakeet frontend, feature-major (n_mels, cols)
class BatchLogMelSpectrogram {
public:
    explicit BatchLogMelSpectrogram(const BatchLogMelConfig &cfg = BatchLogMelConfig(), int device = -1) : n_mels_(static_cast<std::size_t>(cfg.n_mels)) {
        detail::check(melspec_blm_create(&b_, device, &cfg), true);
    }
    ~BatchLogMelSpectrogram() { melspec_blm_destroy(b_); }
    BatchLogMelSpectrogram(const BatchLogMelSpectrogram &) = delete;
    BatchLogMelSpectrogram &operator=(const BatchLogMelSpectrogram &) = delete;

    Array2f compute(const std::vector<float> &samples) {
        Array2f a;
        a.rows = n_mels_;
        a.cols = melspec_blm_padded_frames(b_, samples.size());
        a.data.assign(a.rows * a.cols, 0.0f);
        std::size_t rows = 0, cols = 0;
        detail::check(melspec_blm_compute_host(b_, samples.data(), samples.size(), a.data.data(), a.data.size(), &rows, &cols), false);
        return a;
    }

    // additive: the split output (melspec_hip.h) -- un-normalised rows + per-feature mean and 1 / (std + 1e-5); the consumer applies
    // (x - mean) * inv_std on the valid columns
    bool supports_split() const { return melspec_blm_supports_split(b_) != 0; }
    void compute_uniform_device_split(const float *d_pcm, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, float *d_rows,
                                      float *d_mean, float *d_inv_std, void *stream = nullptr) {
        detail::check(melspec_blm_compute_uniform_device_split(b_, d_pcm, clip_stride, clip_len, n_clips, d_rows, d_mean, d_inv_std, stream), false);
    }
    // the ragged form: clip c = d_pcm[offsets[c] .. + lengths[c]) -> rows [n_mels][cols_c] at d_rows + rows_offsets[c] (nullptr: packed in
    // clip order), mean / inv_std [n_clips][n_mels] -- per clip the bits of the uniform call on that clip alone
    void compute_ragged_device_split(const float *d_pcm, const std::uint64_t *offsets, const std::uint64_t *lengths, std::uint32_t n_clips, float *d_rows,
                                     const std::uint64_t *rows_offsets, float *d_mean, float *d_inv_std, void *stream = nullptr) {
        detail::check(melspec_blm_compute_ragged_device_split(b_, d_pcm, offsets, lengths, n_clips, d_rows, rows_offsets, d_mean, d_inv_std, stream), false);
    }
    // the ragged batch with its clip table in device memory (melspec_blm_compute_ragged_device_desc): u64 offsets / lengths / output offsets
    // (nullptr: packed) on the device, a planner kernel instead of host tables; max_total_columns / max_clip_samples bound what the table
    // may ask for, *d_rejected (device, may be nullptr) receives the number of rejected clips
    bool supports_desc() const { return melspec_blm_supports_desc(b_) != 0; }
    void compute_ragged_device_desc(const float *d_pcm, const std::uint64_t *d_offsets, const std::uint64_t *d_lengths, std::uint32_t n_clips, float *d_out,
                                    const std::uint64_t *d_out_offsets, std::uint64_t max_total_columns, std::uint64_t max_clip_samples,
                                    std::uint32_t *d_rejected = nullptr, void *stream = nullptr) {
        detail::check(melspec_blm_compute_ragged_device_desc(b_, d_pcm, d_offsets, d_lengths, n_clips, d_out, d_out_offsets, max_total_columns, max_clip_samples,
                                                             d_rejected, stream), false);
    }
    struct Split {
        Array2f rows;                      // (n_mels, cols), un-normalised
        std::vector<float> mean, inv_std;  // (n_mels)
    };
    Split compute_split(const std::vector<float> &samples) {
        Split s;
        s.rows.rows = n_mels_;
        s.rows.cols = melspec_blm_padded_frames(b_, samples.size());
        s.rows.data.assign(s.rows.rows * s.rows.cols, 0.0f);
        s.mean.assign(n_mels_, 0.0f);
        s.inv_std.assign(n_mels_, 0.0f);
        std::size_t rows = 0, cols = 0;
        detail::check(melspec_blm_compute_host_split(b_, samples.data(), samples.size(), s.rows.data.data(), s.rows.data.size(), s.mean.data(), s.inv_std.data(),
                                                     &rows, &cols), false);
        return s;
    }

    // additive: the split output with 16-bit ends (melspec_hip.h) -- int16 PCM in, f16 / bf16 rows out (the f32 split call's rows rounded
    // once), f32 mean and inv_std (the f32 split call's bits); strides, offsets and capacities count elements
    bool supports_split_io(int pcm_dtype, int out_dtype) const { return melspec_blm_supports_split_io(b_, pcm_dtype, out_dtype) != 0; }
    void compute_uniform_device_split_io(const void *d_pcm, int pcm_dtype, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, void *d_rows,
                                         int out_dtype, float *d_mean, float *d_inv_std, void *stream = nullptr) {
        detail::check(melspec_blm_compute_uniform_device_split_io(b_, d_pcm, pcm_dtype, clip_stride, clip_len, n_clips, d_rows, out_dtype, d_mean, d_inv_std, stream), false);
    }
    void compute_ragged_device_split_io(const void *d_pcm, int pcm_dtype, const std::uint64_t *offsets, const std::uint64_t *lengths, std::uint32_t n_clips,
                                        void *d_rows, int out_dtype, const std::uint64_t *rows_offsets, float *d_mean, float *d_inv_std, void *stream = nullptr) {
        detail::check(melspec_blm_compute_ragged_device_split_io(b_, d_pcm, pcm_dtype, offsets, lengths, n_clips, d_rows, out_dtype, rows_offsets, d_mean, d_inv_std,
                                                                 stream), false);
    }
    struct SplitS16 {
        std::vector<std::uint16_t> rows;   // (n_mels, cols) row-major, the bit patterns of out_dtype, un-normalised
        std::size_t cols = 0;
        std::vector<float> mean, inv_std;  // (n_mels)
    };
    SplitS16 compute_split_s16(const std::vector<std::int16_t> &samples, int out_dtype) {
        SplitS16 s;
        s.rows.assign(n_mels_ * melspec_blm_padded_frames(b_, samples.size()), 0);
        s.mean.assign(n_mels_, 0.0f);
        s.inv_std.assign(n_mels_, 0.0f);
        std::size_t rows = 0;
        detail::check(melspec_blm_compute_host_split_io(b_, samples.data(), MELSPEC_PCM_S16, samples.size(), s.rows.data(), out_dtype, s.rows.size(), s.mean.data(),
                                                        s.inv_std.data(), &rows, &s.cols), false);
        return s;
    }

    // additive: 16-bit ends (MELSPEC_PCM_*, MELSPEC_OUT_* of melspec_hip.h); strides, offsets and lengths count elements
    bool supports_io(int pcm_dtype, int out_dtype) const { return melspec_blm_supports_io(b_, pcm_dtype, out_dtype) != 0; }
    void compute_uniform_device_io(const void *d_pcm, int pcm_dtype, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, void *d_out,
                                   int out_dtype, void *stream = nullptr) {
        detail::check(melspec_blm_compute_uniform_device_io(b_, d_pcm, pcm_dtype, clip_stride, clip_len, n_clips, d_out, out_dtype, stream), false);
    }
    void compute_ragged_device_io(const void *d_pcm, int pcm_dtype, const std::vector<std::uint64_t> &offsets, const std::vector<std::uint64_t> &lengths,
                                  void *d_out, int out_dtype, const std::uint64_t *out_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_blm_compute_ragged_device_io(b_, d_pcm, pcm_dtype, offsets.data(), lengths.data(), static_cast<std::uint32_t>(offsets.size()), d_out,
                                                           out_dtype, out_offsets, stream), false);
    }
    // compute() on 16-bit PCM (value = sample / 32768, exactly) into out_dtype features (MELSPEC_OUT_F16 / _BF16), returned as their bit
    // patterns, (n_mels, cols) row-major: the int16 bytes are what crosses the bus
    std::vector<std::uint16_t> compute_s16(const std::vector<std::int16_t> &samples, int out_dtype, std::size_t *cols = nullptr) {
        std::vector<std::uint16_t> out(n_mels_ * melspec_blm_padded_frames(b_, samples.size()));
        std::size_t r = 0, c = 0;
        detail::check(melspec_blm_compute_host_io(b_, samples.data(), MELSPEC_PCM_S16, samples.size(), out.data(), out_dtype, out.size(), &r, &c), false);
        if (cols) *cols = c;
        return out;
    }
    void synchronize(void *stream = nullptr) { detail::check(melspec_blm_synchronize(b_, stream), false); }
    void release_scratch() { detail::check(melspec_blm_release_scratch(b_), false); }

private:
    friend class BlmStreamBank;
    melspec_blm *b_ = nullptr;
    std::size_t n_mels_ = 0;
};

// BatchLogMelSpectrogram::compute fed chunk by chunk (melspec_blm_stream_*): after pushes whose chunks concatenate to x and one finish a
// stream has emitted exactly the columns of compute(x) with normalize_per_feature off, un-normalised whatever the object's setting;
// stats() gives the running per-feature mean and 1 / (std + 1e-5) of those columns.  The frontend must outlive the bank.
class BlmStreamBank {
public:
    BlmStreamBank(BatchLogMelSpectrogram &blm, std::size_t n_streams, std::size_t max_chunk) : n_mels_(blm.n_mels_) {
        detail::check(melspec_blm_stream_create(&st_, blm.b_, static_cast<std::uint32_t>(n_streams), static_cast<std::uint32_t>(max_chunk)), true);
    }
    ~BlmStreamBank() { melspec_blm_stream_destroy(st_); }
    BlmStreamBank(const BlmStreamBank &) = delete;
    BlmStreamBank &operator=(const BlmStreamBank &) = delete;

    void reset() { detail::check(melspec_blm_stream_reset(st_, nullptr, 0), false); }
    void reset(const std::vector<std::uint32_t> &ids) { detail::check(melspec_blm_stream_reset(st_, ids.data(), static_cast<std::uint32_t>(ids.size())), false); }
    std::size_t frames_after(std::uint32_t id, std::size_t n_new) const { return melspec_blm_stream_frames_after(st_, id, static_cast<std::uint32_t>(n_new)); }
    std::size_t finish_frames(std::uint32_t id) const { return melspec_blm_stream_finish_frames(st_, id); }
    // one chunk for one stream: the columns it completes, (n_mels, frames) row-major
    Array2f push(std::uint32_t id, const std::vector<float> &chunk) { return push_typed(id, chunk.data(), MELSPEC_PCM_F32, chunk.size()); }
    Array2f push(std::uint32_t id, const std::vector<std::int16_t> &chunk) { return push_typed(id, chunk.data(), MELSPEC_PCM_S16, chunk.size()); }
    // end of the stream: the zero-padded columns; the stream takes no push until reset
    Array2f finish(std::uint32_t id) {
        Array2f a;
        a.rows = n_mels_;
        a.data.assign(finish_frames(id) * n_mels_, 0.0f);
        std::uint32_t got = 0;
        detail::check(melspec_blm_stream_finish_host(st_, &id, 1, a.data.data(), a.data.size(), &got), false);
        a.cols = got;
        return a;
    }
    float *input_ptr(std::uint32_t id) { return melspec_blm_stream_input_ptr(st_, id); }
    void push_device(const std::vector<std::uint32_t> &ids, const void *d_chunks, int pcm_dtype, const std::uint64_t *src_offsets, const std::vector<std::uint32_t> &lens,
                     float *d_out, const std::uint64_t *out_offsets, std::uint32_t *frames_out, void *stream = nullptr) {
        detail::check(melspec_blm_stream_push_device(st_, ids.data(), d_chunks, pcm_dtype, src_offsets, lens.data(), static_cast<std::uint32_t>(ids.size()), d_out,
                                                     out_offsets, frames_out, stream), false);
    }
    void finish_device(const std::vector<std::uint32_t> &ids, float *d_out, const std::uint64_t *out_offsets, std::uint32_t *frames_out, void *stream = nullptr) {
        detail::check(melspec_blm_stream_finish_device(st_, ids.data(), static_cast<std::uint32_t>(ids.size()), d_out, out_offsets, frames_out, stream), false);
    }
    struct Stats {
        std::vector<float> mean, inv_std;  // (n_mels)
        std::uint64_t count = 0;           // columns emitted so far
    };
    Stats stats(std::uint32_t id) {
        Stats s;
        s.mean.assign(n_mels_, 0.0f);
        s.inv_std.assign(n_mels_, 0.0f);
        detail::check(melspec_blm_stream_stats_host(st_, &id, 1, s.mean.data(), s.inv_std.data(), &s.count), false);
        return s;
    }
    void stats_device(const std::vector<std::uint32_t> &ids, float *d_mean, float *d_inv_std, std::uint64_t *counts, void *stream = nullptr) {
        detail::check(melspec_blm_stream_stats_device(st_, ids.data(), static_cast<std::uint32_t>(ids.size()), d_mean, d_inv_std, counts, stream), false);
    }

    // additive: f16 / bf16 rows out (MELSPEC_OUT_* of melspec_hip.h); offsets count elements of the row type, stats() stays that of the f32 rows
    bool supports_io(int pcm_dtype, int out_dtype) const { return melspec_blm_stream_supports_io(st_, pcm_dtype, out_dtype) != 0; }
    // push() on 16-bit PCM / finish() into out_dtype columns (MELSPEC_OUT_F16 / _BF16), returned as their bit patterns, (n_mels, frames) row-major
    std::vector<std::uint16_t> push_s16(std::uint32_t id, const std::vector<std::int16_t> &chunk, int out_dtype, std::size_t *frames = nullptr) {
        std::vector<std::uint16_t> out(frames_after(id, chunk.size()) * n_mels_);
        const std::uint32_t len = static_cast<std::uint32_t>(chunk.size());
        std::uint32_t got = 0;
        detail::check(melspec_blm_stream_push_host_io(st_, &id, chunk.data(), MELSPEC_PCM_S16, &len, 1, out.data(), out_dtype, out.size(), &got), false);
        if (frames) *frames = got;
        return out;
    }
    std::vector<std::uint16_t> finish_io(std::uint32_t id, int out_dtype, std::size_t *frames = nullptr) {
        std::vector<std::uint16_t> out(finish_frames(id) * n_mels_);
        std::uint32_t got = 0;
        detail::check(melspec_blm_stream_finish_host_io(st_, &id, 1, out.data(), out_dtype, out.size(), &got), false);
        if (frames) *frames = got;
        return out;
    }
    void push_device_io(const std::vector<std::uint32_t> &ids, const void *d_chunks, int pcm_dtype, const std::uint64_t *src_offsets,
                        const std::vector<std::uint32_t> &lens, void *d_out, int out_dtype, const std::uint64_t *out_offsets, std::uint32_t *frames_out,
                        void *stream = nullptr) {
        detail::check(melspec_blm_stream_push_device_io(st_, ids.data(), d_chunks, pcm_dtype, src_offsets, lens.data(), static_cast<std::uint32_t>(ids.size()), d_out,
                                                        out_dtype, out_offsets, frames_out, stream), false);
    }
    void finish_device_io(const std::vector<std::uint32_t> &ids, void *d_out, int out_dtype, const std::uint64_t *out_offsets, std::uint32_t *frames_out,
                          void *stream = nullptr) {
        detail::check(melspec_blm_stream_finish_device_io(st_, ids.data(), static_cast<std::uint32_t>(ids.size()), d_out, out_dtype, out_offsets, frames_out, stream), false);
    }

private:
    Array2f push_typed(std::uint32_t id, const void *samples, int pcm_dtype, std::size_t n) {
        Array2f a;
        const std::uint32_t len = static_cast<std::uint32_t>(n);
        a.rows = n_mels_;
        a.data.assign(frames_after(id, n) * n_mels_, 0.0f);
        std::uint32_t got = 0;
        detail::check(melspec_blm_stream_push_host(st_, &id, samples, pcm_dtype, &len, 1, a.data.data(), a.data.size(), &got), false);
        a.cols = got;
        return a;
    }
    void *st_ = nullptr;
    std::size_t n_mels_;
};

// src/quant.rs: quantize / dequantize / tga_8bit / parse_tga_8bit, same names and return shapes
struct QuantizationRange { float min, max; };

class TgaCodec {
public:
    explicit TgaCodec(int device = -1) { detail::check(melspec_tga_create(&q_, device), true); }
    ~TgaCodec() { melspec_tga_destroy(q_); }
    TgaCodec(const TgaCodec &) = delete;
    TgaCodec &operator=(const TgaCodec &) = delete;

    std::pair<std::vector<std::uint8_t>, QuantizationRange> quantize(const std::vector<float> &frame) {
        std::vector<std::uint8_t> out(frame.size());
        float r[2] = {0.0f, 0.0f};
        detail::check(melspec_quantize_host(q_, frame.data(), frame.size(), out.data(), r), false);
        return {std::move(out), QuantizationRange{r[0], r[1]}};
    }
    std::vector<float> dequantize(const std::vector<std::uint8_t> &data, const QuantizationRange &range) {
        std::vector<float> out(data.size());
        const float r[2] = {range.min, range.max};
        detail::check(melspec_dequantize_host(q_, data.data(), data.size(), r, out.data()), false);
        return out;
    }
    // one TGA per <= 65535-column chunk of the major-row-order [n_mels][width] image
    std::vector<std::vector<std::uint8_t>> tga_8bit(const std::vector<float> &data, std::size_t n_mels) {
        std::uint32_t n = 0;
        std::size_t stride = 0, last = 0;
        detail::check(melspec_tga_layout(static_cast<int>(n_mels), n_mels ? data.size() / n_mels : 0, &n, &stride, &last), false);
        std::vector<std::vector<std::uint8_t>> res;
        if (n == 0) return res;
        std::vector<std::uint8_t> flat(stride * (n - 1) + last);
        std::uint32_t got = 0;
        detail::check(melspec_tga_encode_host(q_, data.data(), data.size(), static_cast<int>(n_mels), flat.data(), flat.size(), &got), false);
        const std::size_t full = 26 + n_mels * 65535;
        for (std::uint32_t c = 0; c < n; ++c)
            res.emplace_back(flat.begin() + c * stride, flat.begin() + c * stride + (c + 1 < n ? full : last));
        return res;
    }
    std::vector<float> parse_tga_8bit(const std::vector<std::uint8_t> &blob) {
        std::vector<float> out(blob.size() > 26 ? blob.size() - 26 : 0);
        std::size_t n = 0;
        detail::check(melspec_tga_decode_host(q_, blob.data(), blob.size(), out.data(), out.size(), &n), false);
        out.resize(n);
        return out;
    }

private:
    melspec_tga *q_ = nullptr;
};

// One live stream with the reference's RingBuffer interface (src/rb.rs:18-121) over a 1-stream bank:
// add_frame() feeds samples, maybe_mel() hands out one (n_mels) column per completed hop.
class RingBuffer {
public:
    RingBuffer(HipMelSpectrogram &mel, std::size_t capacity = 16384) : n_mels_(mel.n_mels()), cap_(capacity) {
        detail::check(melspec_stream_create(&st_, mel.raw(), 1, static_cast<std::uint32_t>(capacity)), true);
    }
    ~RingBuffer() { melspec_stream_destroy(st_); }
    RingBuffer(const RingBuffer &) = delete;
    RingBuffer &operator=(const RingBuffer &) = delete;

    void add_frame(const std::vector<float> &samples) {
        pending_.insert(pending_.end(), samples.begin(), samples.end());
        if (pending_.size() > cap_) pending_.erase(pending_.begin(), pending_.begin() + (pending_.size() - cap_));   // src/rb.rs:60-68
    }
    void add(float sample) { add_frame(std::vector<float>(1, sample)); }
    std::optional<std::vector<float>> maybe_mel() {
        if (next_ == ready_.size() / (n_mels_ ? n_mels_ : 1) && !pending_.empty()) {
            const std::uint32_t id = 0, len = static_cast<std::uint32_t>(pending_.size());
            std::uint32_t frames = 0;
            ready_.assign(melspec_stream_frames_after(st_, 0, len) * n_mels_, 0.0f);
            next_ = 0;
            detail::check(melspec_stream_push_host(st_, &id, pending_.data(), &len, 1, ready_.data(), ready_.size(), &frames), false);
            ready_.resize(static_cast<std::size_t>(frames) * n_mels_);
            pending_.clear();
        }
        if (next_ * n_mels_ >= ready_.size()) return std::nullopt;
        std::vector<float> col(ready_.begin() + next_ * n_mels_, ready_.begin() + (next_ + 1) * n_mels_);
        ++next_;
        return col;
    }

    // additive: 16-bit ends (melspec_stream_*_io; MELSPEC_PCM_*, MELSPEC_OUT_* of melspec_hip.h).  These push at once: feed a stream
    // either through them or through add_frame() / maybe_mel(), not both (samples add_frame() still holds would come after theirs).
    bool supports_io(int pcm_dtype, int out_dtype) const { return melspec_stream_supports_io(st_, pcm_dtype, out_dtype) != 0; }
    // a block of 16-bit PCM (value = sample / 32768, exactly; at most the capacity) -> the rows it completes as out_dtype
    // (MELSPEC_OUT_F16 / _BF16) bit patterns, [frames][n_mels]: the int16 bytes are what crosses the bus
    std::vector<std::uint16_t> push_s16(const std::vector<std::int16_t> &samples, int out_dtype, std::size_t *frames = nullptr) {
        const std::uint32_t id = 0, len = static_cast<std::uint32_t>(samples.size());
        std::uint32_t got = 0;
        std::vector<std::uint16_t> out(melspec_stream_frames_after(st_, 0, len) * n_mels_);
        detail::check(melspec_stream_push_host_io(st_, &id, samples.data(), MELSPEC_PCM_S16, &len, 1, out.data(), out_dtype, out.size(), &got), false);
        out.resize(static_cast<std::size_t>(got) * n_mels_);
        if (frames) *frames = got;
        return out;
    }
    // the pending (< hop) samples zero-padded to a hop: at most one more row, as out_dtype (MELSPEC_OUT_F16 / _BF16) bit patterns
    std::vector<std::uint16_t> flush_io(int out_dtype) {
        const std::uint32_t id = 0;
        std::uint32_t got = 0;
        std::vector<std::uint16_t> out(n_mels_);
        detail::check(melspec_stream_flush_host_io(st_, &id, 1, out.data(), out_dtype, out.size(), &got), false);
        out.resize(static_cast<std::size_t>(got) * n_mels_);
        return out;
    }
    // a chunk of pcm_dtype elements that lies in device memory (d_chunk == nullptr: f32 at the stream's input slot) -> rows of out_dtype
    // at d_out; returns the frames emitted, after the launches have completed
    std::uint32_t push_device_io(const void *d_chunk, int pcm_dtype, std::uint32_t len, void *d_out, int out_dtype, void *stream = nullptr) {
        const std::uint32_t id = 0;
        std::uint32_t got = 0;
        detail::check(melspec_stream_push_device_io(st_, &id, d_chunk, pcm_dtype, nullptr, &len, 1, d_out, out_dtype, nullptr, &got, stream), false);
        return got;
    }

private:
    melspec_stream *st_ = nullptr;
    std::size_t n_mels_, cap_, next_ = 0;
    std::vector<float> pending_, ready_;
};

// src/vad.rs: DetectionSettings, vad_boundaries -> EdgeInfo, vad_on
struct DetectionSettings : melspec_vad_settings {
    DetectionSettings() { melspec_vad_default_settings(this); }                       // 0.98, 11, 5, 2
    DetectionSettings(double min_energy_, int min_y_, int min_x_, int min_mel_) {
        min_energy = min_energy_; min_y = min_y_; min_x = min_x_; min_mel = min_mel_;
    }
};
struct EdgeInfo {
    std::vector<std::size_t> non_intersected_columns, intersected_columns;
    std::uint32_t longest_run = 0;
    const std::vector<std::size_t> &non_intersected() const { return non_intersected_columns; }
    const std::vector<std::size_t> &intersected() const { return intersected_columns; }
};
// one (n_mels x width) image, row-major (the reference concatenates its Array2 frames along the time axis)
inline EdgeInfo vad_boundaries(const std::vector<float> &image, std::size_t n_mels, const DetectionSettings &settings, int device = -1) {
    EdgeInfo e;
    const std::size_t width = n_mels ? image.size() / n_mels : 0;
    std::vector<std::uint8_t> mask(melspec_vad_mask_len(static_cast<int>(n_mels), width));
    detail::check(melspec_vad_boundaries_host(device, image.data(), static_cast<int>(n_mels), width, &settings, nullptr, mask.data(),
                                              &e.longest_run), false);
    for (std::size_t x = 0; x < mask.size(); ++x) (mask[x] ? e.intersected_columns : e.non_intersected_columns).push_back(x);
    return e;
}
inline bool vad_on(const EdgeInfo &e, std::size_t n) {          // src/vad.rs:229-254
    return n <= 1 ? e.intersected_columns.size() >= 2 : e.longest_run >= n;
}

// VoiceActivity (src/vad.rs:125-135) and the detector behind a live stream: VoiceActivityDetector::add_activity
// (src/vad.rs:155-205) fed by RingBuffer's frames, with both on the device -- one bank stream whose detector stage is on.
struct VoiceActivity {
    bool active;
    std::size_t frame_index, leading_active_columns, active_columns, window_columns;
    double confidence;
};
class StreamDetector {
public:
    StreamDetector(HipMelSpectrogram &mel, const DetectionSettings &settings, std::size_t max_chunk = 16384) : n_mels_(mel.n_mels()) {
        detail::check(melspec_stream_create(&st_, mel.raw(), 1, static_cast<std::uint32_t>(max_chunk)), true);
        const int rc = melspec_stream_enable_vad(st_, &settings);
        if (rc) { melspec_stream_destroy(st_); st_ = nullptr; detail::check(rc, true); }
    }
    ~StreamDetector() { melspec_stream_destroy(st_); }
    StreamDetector(const StreamDetector &) = delete;
    StreamDetector &operator=(const StreamDetector &) = delete;

    // Feeds samples (any length <= max_chunk); one entry per frame they complete: std::nullopt where add_activity returns None.
    // rows (optional) receives the mel rows of those frames, [frame][n_mels].
    std::vector<std::optional<VoiceActivity>> add_frame(const std::vector<float> &samples, std::vector<float> *rows = nullptr) {
        const std::uint32_t id = 0, len = static_cast<std::uint32_t>(samples.size());
        const std::size_t cap = melspec_stream_frames_after(st_, 0, len);
        const std::uint64_t first = melspec_stream_vad_frames(st_, 0);
        std::vector<float> out(cap * n_mels_);
        std::vector<melspec_vad_activity> acts(cap);
        std::uint32_t frames = 0;
        detail::check(melspec_stream_push_host_vad(st_, &id, samples.data(), &len, 1, out.data(), out.size(), &frames, acts.data(), acts.size()), false);
        std::vector<std::optional<VoiceActivity>> res(frames);
        for (std::uint32_t k = 0; k < frames; ++k) {
            const melspec_vad_activity &a = acts[k];
            if (!a.valid) continue;
            res[k] = VoiceActivity{a.active != 0, static_cast<std::size_t>(first + k), a.leading_active_columns, a.active_columns, a.window_columns,
                                   a.window_columns ? static_cast<double>(a.active_columns) / a.window_columns : 0.0};
        }
        if (rows) { out.resize(static_cast<std::size_t>(frames) * n_mels_); rows->swap(out); }
        return res;
    }

private:
    melspec_stream *st_ = nullptr;
    std::size_t n_mels_;
};

// dense [n_mels][n_fft/2+1] row-major; std::nullopt == None
inline std::vector<double> mel(double sr, std::size_t n_fft, std::size_t n_mels, std::optional<double> f_min = std::nullopt,
                               std::optional<double> f_max = std::nullopt, bool htk = false, bool norm = true) {
    std::vector<double> w(n_mels * (n_fft / 2 + 1));
    detail::check(melspec_mel_filterbank(sr, static_cast<int>(n_fft), static_cast<int>(n_mels), f_min.value_or(-1.0),
                                         f_max.value_or(-1.0), htk, norm, w.data()), false);
    return w;
}

inline double hz_to_mel(double frequency, bool htk = false) { return melspec_hz_to_mel(frequency, htk); }     // src/mel.rs:591-607
inline double mel_to_hz(double mel_value, bool htk = false) { return melspec_mel_to_hz(mel_value, htk); }      // src/mel.rs:609-625
inline std::vector<double> mel_frequencies(std::size_t n_mels, double fmin, double fmax, bool htk = false) {   // src/mel.rs:631-637
    std::vector<double> f(n_mels);
    detail::check(melspec_mel_frequencies(static_cast<int>(n_mels), fmin, fmax, htk, f.data()), false);
    return f;
}
inline std::vector<double> fft_frequencies(double sr, std::size_t n_fft) {                                     // src/mel.rs:639-643
    std::vector<double> f(n_fft / 2 + 1);
    detail::check(melspec_fft_frequencies(sr, static_cast<int>(n_fft), f.data()), false);
    return f;
}

}  // namespace melspec
