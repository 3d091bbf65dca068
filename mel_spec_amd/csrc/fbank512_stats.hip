// fbank512_stats.hip -- the NeMo / Parakeet frontend's split output (fbank512_stats_kernels.hpp): the f64 kernel (eight waves) and the f32
// kernel (twelve waves, staged rows) of the compile-time 80- and 128-mel Slaney banks with the per-block partials of the row statistics,
// and the kernel that merges a clip's partials into mean and 1 / (std + 1e-5).  Kept out of fbank512.hip so that its kernels stay the
// instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_stats_kernels.hpp"

namespace melspec {

template __global__ void fbank512_nemo_stats_kernel<double, 8, kBlmSlots, LensSlaney128>(const FbankStatsParams);
template __global__ void fbank512_nemo_stats_kernel<double, 8, kFbSlots, LensSlaney80>(const FbankStatsParams);
template __global__ void fbank512_nemo_stats_kernel<float, 12, kBlmSlots, LensSlaney128>(const FbankStatsParams);
template __global__ void fbank512_nemo_stats_kernel<float, 12, kFbSlots, LensSlaney80>(const FbankStatsParams);

// One thread per (clip, mel): the clip's partials in block order, merged in f64, rounded once.  The statistics of normalize_per_feature
// (src/mel.rs:721-749): mean over the valid frames, unbiased variance with the denominator max(valid - 1, 1), 1 / (sqrt(var) + 1e-5).
__global__ __launch_bounds__(kBlmStatsFinishThreads) void blm_stats_finish_kernel(const BlmStatsFinishParams p) {
    const uint64_t rows = static_cast<uint64_t>(p.n_clips) * p.n_mels;
    const uint64_t blocks = (p.valid + p.block_frames - 1) / p.block_frames;
    for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kBlmStatsFinishThreads + threadIdx.x; row < rows; row += static_cast<uint64_t>(gridDim.x) * kBlmStatsFinishThreads) {
        const uint64_t clip = row / p.n_mels, m = row - clip * p.n_mels;
        const float2 *part = p.part + clip * p.blocks_per_clip * static_cast<uint64_t>(p.n_mels) + m;
        double mean = 0.0, M2 = 0.0, n = 0.0;
        for (uint64_t b = 0; b < blocks; ++b) {
            const uint64_t left = p.valid - b * p.block_frames;
            const float2 u = part[b * p.n_mels];
            stats_merge(mean, M2, n, static_cast<double>(u.x), static_cast<double>(u.y), static_cast<double>(left < p.block_frames ? left : p.block_frames));
        }
        const double denom = p.valid > 1 ? static_cast<double>(p.valid - 1) : 1.0;
        p.mean[row] = static_cast<float>(mean);
        p.inv_std[row] = static_cast<float>(1.0 / (__builtin_sqrt(M2 / denom) + static_cast<double>(1e-5f)));
    }
}

}  // namespace melspec
