// fbank512_stats_io.hip -- the NeMo / Parakeet frontend's split output with int16 PCM in and / or f16 / bf16 rows out, uniform and ragged
// batches (fbank512_stats_io_kernels.hpp): per kernel of the f32 split call (MS_K512_STATS: the f64 kernel on eight waves and the f32
// kernel on twelve, 80- and 128-mel Slaney bank) the five (sample, row) combinations, and the table that finds them.  A unit of its own so
// that the kernels of fbank512_stats.hip, fbank512_stats_ragged.hip and fbank512_io.hip stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_stats_io_kernels.hpp"
#include "blm_split_io_plan.hpp"

namespace melspec {

// one row of five per stats kernel, in the order of io_index() (MS_K512_IO5's)
#define MS_STATS_IO_ROW(name, T, W, N, L) MS_K512_IO5(MS_STATS_IO_X, name, T, W, N, L)

#define MS_STATS_IO_X(name, In, Out, T, W, N, L) template __global__ void fbank512_nemo_stats_io_kernel<T, W, N, L, In, Out>(const FbankStatsRaggedParams);
MS_K512_STATS(MS_STATS_IO_ROW)
#undef MS_STATS_IO_X

namespace {
#define MS_STATS_IO_X(name, In, Out, T, W, N, L) &fbank512_nemo_stats_io_kernel<T, W, N, L, In, Out>,
const FbankStatsIoKernel kStatsIoKernels[] = {MS_K512_STATS(MS_STATS_IO_ROW)};
#undef MS_STATS_IO_X
static_assert(sizeof(kStatsIoKernels) / sizeof(kStatsIoKernels[0]) == host::kBlmSplitIoKernels, "five kernels per stats kernel, in the order of the lists");
}  // namespace
#undef MS_STATS_IO_ROW

FbankStatsIoKernel nemo_stats_io_kernel(host::K512 stats, int io) {
    const int at = host::blm_split_io_slot(stats, io);
    return at < 0 ? nullptr : kStatsIoKernels[at];
}

}  // namespace melspec
