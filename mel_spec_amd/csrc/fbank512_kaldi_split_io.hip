// fbank512_kaldi_split_io.hip -- the Kaldi fbank's split output with int16 PCM in and / or f16 / bf16 rows out, uniform and ragged batches
// (fbank512_kaldi_split_io_kernels.hpp): the workgroup-per-clip kernel of the compile-time 80-bin Kaldi bank in its five (sample, row)
// combinations, each for equal clips and for clips handed out by the plan's order, and the table that finds them.  A unit of its own so that
// the kernels of fbank512.hip and fbank512_kaldi_io.hip stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_kaldi_split_io_kernels.hpp"
#include "fbank_split_io_plan.hpp"

namespace melspec {

// one row of five per kind of batch, in the order of io_index() (MS_K512_IO5's)
#define MS_SPLIT_IO_ROWS(X) MS_K512_IO5(X, kUniform, false) MS_K512_IO5(X, kRagged, true)

#define MS_SPLIT_IO_X(name, In, Out, R) template __global__ void fbank512_clip_split_io_kernel<kFbSlots, LensKaldi80, In, Out, R>(const FbankClipParams);
MS_SPLIT_IO_ROWS(MS_SPLIT_IO_X)
#undef MS_SPLIT_IO_X

namespace {
#define MS_SPLIT_IO_X(name, In, Out, R) &fbank512_clip_split_io_kernel<kFbSlots, LensKaldi80, In, Out, R>,
const FbankClipSplitIoKernel kSplitIoKernels[] = {MS_SPLIT_IO_ROWS(MS_SPLIT_IO_X)};
#undef MS_SPLIT_IO_X
static_assert(sizeof(kSplitIoKernels) / sizeof(kSplitIoKernels[0]) == host::kFbankSplitIoKernels, "five kernels per kind of batch, in the order of the lists");
}  // namespace
#undef MS_SPLIT_IO_ROWS

FbankClipSplitIoKernel kaldi_split_io_kernel(bool ragged, int io) {
    const int at = host::fbank_split_io_slot(ragged, io);
    return at < 0 ? nullptr : kSplitIoKernels[at];
}

}  // namespace melspec
