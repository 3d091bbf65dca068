// fbank512_stream_kernels.hpp -- the kernels of the Kaldi fbank's stream bank (melspec_fbank_stream_*): Fbank::compute (src/fbank.rs:141-236)
// fed chunk by chunk, rows before CMN plus running column sums.
//   fbank512_stream_kernel: the body of fbank512_wave_kernel's Kaldi flavour (the same text, included again with MS_FB512_CONTINUES) with
//     the template arguments of the kernel a plain batch of the same object runs on: same arithmetic, same stores, so a stream's rows are
//     the bits of the batch call on its concatenated samples.  A clip of the plan is one stream's push: the frames it completes, read in
//     place from carry ++ chunk in the bank's state.  The one difference is which frame has no predecessor sample: the batch kernels say
//     "the first frame of a clip" (src/fbank.rs:177-181, start == 0); here that is the first frame of a STREAM, and a push that continues
//     one (d_cont[clip] != 0) pre-emphasises its first sample with the sample in front of it like any other frame.  The Povey window is 0
//     there, so for finite input the product vanishes either way; a NaN or an infinity in that place makes the frame NaN in the reference
//     and has to make it NaN here.  A stream's very first frame never reads in front of its samples.
//   fbank_stream_sum_kernel: behind the frame kernel, one workgroup per pushed stream: a lane per mel bin adds the push's rows, in frame
//     order, to the stream's f64 column sums -- a left fold over the stream's frames whatever the chunking -- and lane 0 the frame count.
//   fbank_stream_mean_kernel: mean[bin] = (float)(sum / count) of the listed streams (0 for a stream without a frame).
// Instantiated in a translation unit of their own (fbank512_stream.hip): the kernels that exist keep the instructions they have.
#pragma once
#include "fbank512_kernels.hpp"
#include "stream_plan.hpp"

namespace melspec {

struct FbankStreamParams {
    FbankFastParams f;          // a ragged plain batch over the bank's state: clip i = entry i of the push
    const uint32_t *d_cont;     // [n_clips]: the clip's first frame has a predecessor sample
};

template <class T, int WAVES, int NSLOTS, class Lens, bool RUNS>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_stream_kernel(const FbankStreamParams q) {
    constexpr int FLAVOR = kFlavorKaldi;
    const FbankFastParams &p = q.f;
#define MS_FB512_IN float
#define MS_FB512_OUT float
#define MS_FB512_CONTINUES 1
#include "fbank512_wave_body.inc"
#undef MS_FB512_CONTINUES
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

struct FbankStreamSumParams {
    const StreamEntry *entries; // the push: stream, frames, out_off (first float of the entry's rows)
    const float *rows;
    double *sums;               // [n_streams][n_mels]
    unsigned long long *counts; // [n_streams]
    int n_mels;
};
struct FbankStreamMeanParams {
    const uint32_t *ids;        // [n]
    const double *sums;
    const unsigned long long *counts;
    float *means;               // [n][n_mels]
    uint32_t n;
    int n_mels;
};
constexpr int kFbankStreamSumThreads = 128;
__global__ void fbank_stream_sum_kernel(const FbankStreamSumParams p);        // fbank512_stream.hip
__global__ void fbank_stream_mean_kernel(const FbankStreamMeanParams p);

}  // namespace melspec
