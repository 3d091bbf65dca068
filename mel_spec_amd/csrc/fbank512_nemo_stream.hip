// fbank512_nemo_stream.hip -- the NeMo / Parakeet frontend's stream bank (fbank512_nemo_stream_kernels.hpp): the NeMo flavour of the
// wave-owned kernels with a window origin per clip -- the f64 kernels of the 128-mel, 80-mel and run-time banks on eight waves, of the
// run-time banks on four, and the f32 kernels of the compile-time banks on twelve --, the running statistics and their read-out.
// Kept out of fbank512.hip so that its kernels stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_nemo_stream_kernels.hpp"

namespace melspec {

#define MS_NEMO_STREAM_INST(name, T, W, N, L) template __global__ void fbank512_nemo_stream_kernel<T, W, N, L>(const FbankNemoStreamParams);
MS_K512_NEMO_STREAM(MS_NEMO_STREAM_INST)
#undef MS_NEMO_STREAM_INST

FbankNemoStreamKernel nemo_stream_kernel(host::K512 batch_kernel) {
    switch (batch_kernel) {
#define MS_NEMO_STREAM_CASE(name, T, W, N, L) case host::K512::name: return &fbank512_nemo_stream_kernel<T, W, N, L>;
        MS_K512_NEMO_STREAM(MS_NEMO_STREAM_CASE)
#undef MS_NEMO_STREAM_CASE
        default: return nullptr;
    }
}

// One workgroup per entry of the push, a lane per mel row: Welford's update with the entry's columns in time order, in f64 and without
// contraction (every operation rounds once, as written).  One writer per word (a stream appears once per push, pushes of a bank are in
// stream order): plain loads and stores.
__global__ __launch_bounds__(kBlmStreamStatsThreads) void blm_stream_stats_kernel(const BlmStreamStatsParams p) {
#pragma clang fp contract(off)
    const StreamEntry e = p.entries[blockIdx.x];
    if (e.frames == 0) return;
    const float *rows = p.rows + e.out_off;
    double *mom = p.moments + static_cast<uint64_t>(e.stream) * 2 * p.n_mels;
    const unsigned long long c0 = p.counts[e.stream];
    for (int m = threadIdx.x; m < p.n_mels; m += kBlmStreamStatsThreads) {
        const float *row = rows + static_cast<uint64_t>(m) * e.frames;
        double mean = mom[m], M2 = mom[p.n_mels + m];
        for (uint32_t f = 0; f < e.frames; ++f) {
            const double x = static_cast<double>(row[f]);
            const double d = x - mean;
            mean = mean + d / static_cast<double>(c0 + f + 1);
            M2 = M2 + d * (x - mean);
        }
        mom[m] = mean;
        mom[p.n_mels + m] = M2;
    }
    __syncthreads();                     // every lane has read the count
    if (threadIdx.x == 0) p.counts[e.stream] = c0 + e.frames;
}

__global__ __launch_bounds__(kBlmStreamStatsThreads) void blm_stream_moments_kernel(const BlmStreamMomentsParams p) {
#pragma clang fp contract(off)
    const uint64_t total = static_cast<uint64_t>(p.n) * p.n_mels;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kBlmStreamStatsThreads + threadIdx.x; i < total; i += static_cast<uint64_t>(gridDim.x) * kBlmStreamStatsThreads) {
        const uint64_t k = i / p.n_mels, m = i - k * p.n_mels;
        const uint32_t s = p.ids[k];
        const unsigned long long c = p.counts[s];
        const double *mom = p.moments + static_cast<uint64_t>(s) * 2 * p.n_mels;
        const double denom = c > 1 ? static_cast<double>(c - 1) : 1.0;
        p.mean[i] = c ? static_cast<float>(mom[m]) : 0.0f;
        p.inv_std[i] = static_cast<float>(1.0 / (sqrt((c ? mom[p.n_mels + m] : 0.0) / denom) + 1e-5));
    }
}

}  // namespace melspec
