// fbank512_stream.hip -- the Kaldi fbank's stream bank (fbank512_stream_kernels.hpp): the wave-owned f64 kernels of the 80-bin, 40-bin and
// run-time banks on eight waves and of the run-time bank on four, with the per-clip "continues" flag; the column sums and their means.
// Kept out of fbank512.hip so that its kernels stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_stream_kernels.hpp"
#include "fused512_route.hpp"

namespace melspec {

#define MS_STREAM_INST(name, T, W, N, L, R) template __global__ void fbank512_stream_kernel<T, W, N, L, R>(const FbankStreamParams);
MS_K512_STREAM(MS_STREAM_INST)
#undef MS_STREAM_INST

// One workgroup per entry of the push, a lane per mel bin: sums[stream][bin] += row[f][bin] for the entry's frames f in order, in f64.
// One writer per word (a stream appears once per push, pushes of a bank are in stream order): plain loads and stores.
__global__ __launch_bounds__(kFbankStreamSumThreads) void fbank_stream_sum_kernel(const FbankStreamSumParams p) {
    const StreamEntry e = p.entries[blockIdx.x];
    if (e.frames == 0) return;
    const float *rows = p.rows + e.out_off;
    double *sums = p.sums + static_cast<uint64_t>(e.stream) * p.n_mels;
    for (int m = threadIdx.x; m < p.n_mels; m += kFbankStreamSumThreads) {
        double s = sums[m];
        for (uint32_t f = 0; f < e.frames; ++f) s += static_cast<double>(rows[static_cast<uint64_t>(f) * p.n_mels + m]);
        sums[m] = s;
    }
    if (threadIdx.x == 0) p.counts[e.stream] += e.frames;
}

__global__ __launch_bounds__(kFbankStreamSumThreads) void fbank_stream_mean_kernel(const FbankStreamMeanParams p) {
    const uint64_t total = static_cast<uint64_t>(p.n) * p.n_mels;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kFbankStreamSumThreads + threadIdx.x; i < total; i += static_cast<uint64_t>(gridDim.x) * kFbankStreamSumThreads) {
        const uint64_t k = i / p.n_mels, m = i - k * p.n_mels;
        const uint32_t s = p.ids[k];
        const unsigned long long c = p.counts[s];
        p.means[i] = c ? static_cast<float>(p.sums[static_cast<uint64_t>(s) * p.n_mels + m] / static_cast<double>(c)) : 0.0f;
    }
}

}  // namespace melspec
