// fbank512_stats_ragged.hip -- the ragged form of the NeMo / Parakeet frontend's split output (fbank512_stats_ragged_kernels.hpp): the f64
// kernel (eight waves) and the f32 kernel (twelve waves, staged rows) of the compile-time 80- and 128-mel Slaney banks over a ragged
// batch, and the kernel that merges each clip's partials into mean and 1 / (std + 1e-5).  A unit of its own so that the kernels of
// fbank512.hip and fbank512_stats.hip stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_stats_ragged_kernels.hpp"

namespace melspec {

template __global__ void fbank512_nemo_stats_ragged_kernel<double, 8, kBlmSlots, LensSlaney128>(const FbankStatsRaggedParams);
template __global__ void fbank512_nemo_stats_ragged_kernel<double, 8, kFbSlots, LensSlaney80>(const FbankStatsRaggedParams);
template __global__ void fbank512_nemo_stats_ragged_kernel<float, 12, kBlmSlots, LensSlaney128>(const FbankStatsRaggedParams);
template __global__ void fbank512_nemo_stats_ragged_kernel<float, 12, kFbSlots, LensSlaney80>(const FbankStatsRaggedParams);

// One thread per (clip, mel): blm_stats_finish_kernel's merge -- the clip's partials in block order, in f64, rounded once -- with the
// clip's first block and its valid frames from the batch's tables.
__global__ __launch_bounds__(kBlmStatsFinishThreads) void blm_stats_finish_ragged_kernel(const BlmStatsFinishRaggedParams p) {
    const uint64_t rows = static_cast<uint64_t>(p.n_clips) * p.n_mels;
    for (uint64_t row = static_cast<uint64_t>(blockIdx.x) * kBlmStatsFinishThreads + threadIdx.x; row < rows; row += static_cast<uint64_t>(gridDim.x) * kBlmStatsFinishThreads) {
        const uint64_t clip = row / p.n_mels, m = row - clip * p.n_mels;
        const uint64_t valid = p.d_valid[clip];
        if (valid == 0) continue;
        const uint64_t blocks = (valid + p.block_frames - 1) / p.block_frames;
        const float2 *part = p.part + (p.d_unit_prefix[clip] / p.waves) * static_cast<uint64_t>(p.n_mels) + m;
        double mean = 0.0, M2 = 0.0, n = 0.0;
        for (uint64_t b = 0; b < blocks; ++b) {
            const uint64_t left = valid - b * p.block_frames;
            const float2 u = part[b * p.n_mels];
            stats_merge(mean, M2, n, static_cast<double>(u.x), static_cast<double>(u.y), static_cast<double>(left < p.block_frames ? left : p.block_frames));
        }
        const double denom = valid > 1 ? static_cast<double>(valid - 1) : 1.0;
        p.mean[row] = static_cast<float>(mean);
        p.inv_std[row] = static_cast<float>(1.0 / (__builtin_sqrt(M2 / denom) + static_cast<double>(1e-5f)));
    }
}

}  // namespace melspec
