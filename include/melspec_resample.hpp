// melspec_resample.hpp -- header-only C++ wrapper of the resampler's C ABI (melspec_resample.h), in the style of melspec_hip.hpp: RAII,
// move-only, single-threaded; construction problems throw HipUnavailable, per-call problems HipRuntimeError.
//
//   melspec::Resampler rs(48000, 16000);
//   rs.uniform_device(d_pcm, MELSPEC_PCM_S16, stride, len, n_clips, d_out, rs.out_len(len), stream);      // asynchronous, output stays in HBM
//   std::vector<float> y = rs.compute(samples);                                                           // one host clip, synchronous
#pragma once
#include "melspec_hip.hpp"
#include "melspec_resample.h"

namespace melspec {

struct ResampleGeometry {
    std::uint32_t orig = 0, new_rate = 0, width = 0, max_inside_taps = 0;
    std::uint32_t taps_per_phase() const { return 2 * width + orig; }      // K
};

inline ResampleGeometry resample_geometry(std::uint32_t rate_in, std::uint32_t rate_out) {
    ResampleGeometry g;
    detail::check(melspec_resample_geometry(rate_in, rate_out, &g.orig, &g.new_rate, &g.width, &g.max_inside_taps), false);
    return g;
}
// the dense tap table, [new][K] row-major
inline std::vector<double> resample_taps(std::uint32_t rate_in, std::uint32_t rate_out) {
    const ResampleGeometry g = resample_geometry(rate_in, rate_out);
    std::vector<double> h(static_cast<std::size_t>(g.new_rate) * g.taps_per_phase());
    detail::check(melspec_resample_taps(rate_in, rate_out, h.data(), h.size()), false);
    return h;
}

class Resampler {
public:
    Resampler(std::uint32_t rate_in, std::uint32_t rate_out, int device = -1) : rate_in_(rate_in), rate_out_(rate_out) {
        detail::check(melspec_resampler_create(&r_, device, rate_in, rate_out), true);
    }
    ~Resampler() { melspec_resampler_destroy(r_); }
    Resampler(Resampler &&o) noexcept : r_(std::exchange(o.r_, nullptr)), rate_in_(o.rate_in_), rate_out_(o.rate_out_) {}
    Resampler &operator=(Resampler &&o) noexcept {
        if (this != &o) { melspec_resampler_destroy(r_); r_ = std::exchange(o.r_, nullptr); rate_in_ = o.rate_in_; rate_out_ = o.rate_out_; }
        return *this;
    }
    Resampler(const Resampler &) = delete;
    Resampler &operator=(const Resampler &) = delete;

    std::size_t out_len(std::size_t n_in) const { return melspec_resample_out_len(rate_in_, rate_out_, n_in); }
    std::string kernel_name() const { return melspec_resampler_kernel_name(r_); }

    // device memory in, device memory out, stream-ordered and asynchronous (stream: a hipStream_t, nullptr = the resampler's own)
    void uniform_device(const void *d_pcm, int pcm_dtype, std::uint64_t clip_stride, std::uint64_t clip_len, std::uint32_t n_clips, float *d_out,
                        std::uint64_t out_stride, void *stream = nullptr) {
        detail::check(melspec_resample_uniform_device(r_, d_pcm, pcm_dtype, clip_stride, clip_len, n_clips, d_out, out_stride, stream), false);
    }
    // h_out_offsets == nullptr: packed in clip order
    void ragged_device(const void *d_pcm, int pcm_dtype, const std::uint64_t *h_offsets, const std::uint64_t *h_lengths, std::uint32_t n_clips, float *d_out,
                       const std::uint64_t *h_out_offsets = nullptr, void *stream = nullptr) {
        detail::check(melspec_resample_ragged_device(r_, d_pcm, pcm_dtype, h_offsets, h_lengths, n_clips, d_out, h_out_offsets, stream), false);
    }
    void synchronize(void *stream = nullptr) { detail::check(melspec_resampler_synchronize(r_, stream), false); }

    // one clip from host memory, synchronous
    std::vector<float> compute(const std::vector<float> &samples) { return host(samples.data(), MELSPEC_PCM_F32, samples.size()); }
    std::vector<float> compute(const std::vector<std::int16_t> &samples) { return host(samples.data(), MELSPEC_PCM_S16, samples.size()); }

private:
    std::vector<float> host(const void *samples, int pcm_dtype, std::size_t n) {
        std::vector<float> out(out_len(n));
        std::size_t n_out = 0;
        detail::check(melspec_resample_host(r_, samples, pcm_dtype, n, out.data(), out.size(), &n_out), false);
        out.resize(n_out);
        return out;
    }
    melspec_resampler *r_ = nullptr;
    std::uint32_t rate_in_ = 0, rate_out_ = 0;
};

}  // namespace melspec
