// stream_banks_io.hip -- the stream banks' folds with a 16-bit row store (stream_banks_io_kernels.hpp): the twins of fbank_stream_sum_kernel
// (fbank512_stream.hip) and blm_stream_stats_kernel (fbank512_nemo_stream.hip) behind the typed pushes of the Kaldi fbank's and the NeMo /
// Parakeet frontend's stream banks.  Kept out of those units so that their kernels stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "stream_banks_io_kernels.hpp"

#include "../../include/melspec_hip.h"
#include "fbank512_nemo_stream_kernels.hpp"      // kBlmStreamStatsThreads
#include "fbank512_stream_kernels.hpp"           // kFbankStreamSumThreads
#include "io_types.hpp"
#include "whisper_wave.hpp"                      // row_value

namespace melspec {

// fbank_stream_sum_kernel's fold over the scratch: one workgroup per entry of the push, a lane per mel bin, the entry's frames in order, in
// f64; the element just added goes, rounded once, to the caller's row.  One writer per word of the sums, as there.
template <class Out>
__global__ __launch_bounds__(kFbankStreamSumThreads) void fbank_stream_sum_io_kernel(const FbankStreamSumIoParams p) {
    const StreamEntry e = p.entries[blockIdx.x];
    if (e.frames == 0) return;
    const float *rows = p.rows + p.src_off[blockIdx.x];
    Out *dst = static_cast<Out *>(p.dst) + e.out_off;
    double *sums = p.sums + static_cast<uint64_t>(e.stream) * p.n_mels;
    for (int m = threadIdx.x; m < p.n_mels; m += kFbankStreamSumThreads) {
        double s = sums[m];
        for (uint32_t f = 0; f < e.frames; ++f) {
            const uint64_t i = static_cast<uint64_t>(f) * p.n_mels + m;
            const float x = rows[i];
            s += static_cast<double>(x);
            dst[i] = row_value<Out>(x);
        }
        sums[m] = s;
    }
    if (threadIdx.x == 0) p.counts[e.stream] += e.frames;
}

// blm_stream_stats_kernel's Welford update over the scratch: one workgroup per entry of the push, a lane per mel row, the entry's columns
// in time order, in f64 and without contraction; the element just folded goes, rounded once, to the caller's row.
// The entry's [n_mels][frames] rows go through LDS a tile of p.tile columns at a time, [n_mels][tile + 1] floats: the workgroup loads the
// tile with consecutive lanes on consecutive columns of a mel row, stores it, rounded, the same way -- contiguous 2-byte stores along the
// row instead of a wave's stores `frames` elements apart --, and a lane per mel row folds its row of the tile out of LDS (rows tile + 1
// apart: no bank conflict).  The moments of a mel row pass from tile to tile through the bank's own words, written and read by the one
// lane that owns the row.
template <class Out>
__global__ __launch_bounds__(kBlmStreamStatsThreads) void blm_stream_stats_io_kernel(const BlmStreamStatsIoParams p) {
#pragma clang fp contract(off)
    extern __shared__ float stats_io_tile[];
    const StreamEntry e = p.entries[blockIdx.x];
    if (e.frames == 0) return;
    const float *rows = p.rows + p.src_off[blockIdx.x];
    Out *dst = static_cast<Out *>(p.dst) + e.out_off;
    double *mom = p.moments + static_cast<uint64_t>(e.stream) * 2 * p.n_mels;
    const unsigned long long c0 = p.counts[e.stream];
    const uint32_t pitch = static_cast<uint32_t>(p.tile) + 1;
    for (uint32_t f0 = 0; f0 < e.frames; f0 += p.tile) {
        const uint32_t nf = e.frames - f0 < static_cast<uint32_t>(p.tile) ? e.frames - f0 : static_cast<uint32_t>(p.tile);
        const uint32_t total = static_cast<uint32_t>(p.n_mels) * nf;
        __syncthreads();                 // the previous tile has been folded and stored
        for (uint32_t i = threadIdx.x; i < total; i += kBlmStreamStatsThreads) {
            const uint32_t m = i / nf, f = i - m * nf;
            stats_io_tile[m * pitch + f] = rows[static_cast<uint64_t>(m) * e.frames + f0 + f];
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < total; i += kBlmStreamStatsThreads) {
            const uint32_t m = i / nf, f = i - m * nf;
            dst[static_cast<uint64_t>(m) * e.frames + f0 + f] = row_value<Out>(stats_io_tile[m * pitch + f]);
        }
        for (int m = threadIdx.x; m < p.n_mels; m += kBlmStreamStatsThreads) {
            const float *row = stats_io_tile + static_cast<uint32_t>(m) * pitch;
            double mean = mom[m], M2 = mom[p.n_mels + m];
            for (uint32_t f = 0; f < nf; ++f) {
                const double x = static_cast<double>(row[f]);
                const double d = x - mean;
                mean = mean + d / static_cast<double>(c0 + f0 + f + 1);
                M2 = M2 + d * (x - mean);
            }
            mom[m] = mean;
            mom[p.n_mels + m] = M2;
        }
    }
    __syncthreads();                     // every lane has read the count
    if (threadIdx.x == 0) p.counts[e.stream] = c0 + e.frames;
}

hipError_t fbank_stream_sum_io_launch(const FbankStreamSumIoParams &p, int out_dtype, uint32_t n, hipStream_t s) {
    if (out_dtype == MELSPEC_OUT_F16) hipLaunchKernelGGL(fbank_stream_sum_io_kernel<io_f16>, dim3(n), dim3(kFbankStreamSumThreads), 0, s, p);
    else hipLaunchKernelGGL(fbank_stream_sum_io_kernel<io_bf16>, dim3(n), dim3(kFbankStreamSumThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t blm_stream_stats_io_launch(const BlmStreamStatsIoParams &params, int out_dtype, uint32_t n, hipStream_t s) {
    BlmStreamStatsIoParams p = params;
    // 64 columns per tile (128 bytes of a 16-bit mel row per store), fewer while [n_mels][tile + 1] floats are above 48 KiB of LDS
    p.tile = 64;
    while (p.tile > 1 && static_cast<size_t>(p.n_mels) * (p.tile + 1) * sizeof(float) > 48u * 1024) p.tile >>= 1;
    const size_t lds = static_cast<size_t>(p.n_mels) * (p.tile + 1) * sizeof(float);
    if (out_dtype == MELSPEC_OUT_F16) hipLaunchKernelGGL(blm_stream_stats_io_kernel<io_f16>, dim3(n), dim3(kBlmStreamStatsThreads), lds, s, p);
    else hipLaunchKernelGGL(blm_stream_stats_io_kernel<io_bf16>, dim3(n), dim3(kBlmStreamStatsThreads), lds, s, p);
    return hipGetLastError();
}

}  // namespace melspec
