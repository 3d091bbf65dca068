// fbank512_nemo_stream_kernels.hpp -- the kernels of the NeMo / Parakeet frontend's stream bank (melspec_blm_stream_*):
// BatchLogMelSpectrogram::compute (src/mel.rs) fed chunk by chunk, un-normalised feature-major rows plus the running per-feature
// statistics normalize_per_feature needs.
//   fbank512_nemo_stream_kernel: the body of fbank512_wave_kernel's NeMo flavour (the same text, included again with MS_FB512_CLIP_ORG0)
//     with the template arguments of the kernel a batch of the same object runs on: same arithmetic, same stores, so a stream's columns are
//     the bits of the batch call on its concatenated samples.  A clip of the plan is one stream's push: the frames it completes, read in
//     place from carry ++ chunk in the bank's state.  The one difference is where a clip's first frame starts: a batch has one origin
//     (p.org0: -200 centred, +56 not), a push has one per clip (d_org0[clip]: 1 for a stream in steady state, whose clip begins at the
//     predecessor of the frame's first tap).  The `inside` test and the guarded form (taps outside [0, len) are zero, index 0 is not
//     pre-emphasised) are the batch's: a continuing stream reads index 0 as a predecessor only, and a stream's first samples sit at index 0.
//   blm_stream_stats_kernel: behind the frame kernel, one workgroup per pushed stream, a lane per mel row: Welford's update of the stream's
//     (mean, M2) in f64 with the push's columns in time order -- a left fold over the stream's columns whatever the chunking.  Compiled
//     without contraction: the bits do not depend on how the compiler schedules it.
//   blm_stream_moments_kernel: mean (f32) and 1 / (sqrt(M2 / max(count - 1, 1)) + 1e-5) of the listed streams.
// Instantiated in a translation unit of their own (fbank512_nemo_stream.hip): the kernels that exist keep the instructions they have.
#pragma once
#include "fbank512_kernels.hpp"
#include "fused512_route.hpp"
#include "stream_plan.hpp"

namespace melspec {

struct FbankNemoStreamParams {
    FbankFastParams f;          // a ragged feature-major batch over the bank's state: clip i = entry i of the push (f.org0 is not read)
    const int *d_org0;          // [n_clips]: clip index of tap 0 of the clip's first frame
};

template <class T, int WAVES, int NSLOTS, class Lens>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_nemo_stream_kernel(const FbankNemoStreamParams q) {
    constexpr int FLAVOR = kFlavorNemo;
    constexpr bool RUNS = false;
    const FbankFastParams &p = q.f;
#define MS_FB512_IN float
#define MS_FB512_OUT float
#define MS_FB512_CLIP_ORG0 1
#include "fbank512_wave_body.inc"
#undef MS_FB512_CLIP_ORG0
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

// One per kernel a batch of a NeMo object can run on (the kLayout routes of fused512_route.hpp), named by that kernel:
// X(batch kernel, T, WAVES, NSLOTS, LENS)
#define MS_K512_NEMO_STREAM(X)                                    \
    X(kNemo128, double, 8, kBlmSlots, LensSlaney128)              \
    X(kNemo80, double, 8, kFbSlots, LensSlaney80)                 \
    X(kNemoRt6, double, 8, kFbSlots, LensRuntime)                 \
    X(kNemoRt10, double, 8, kBlmSlots, LensRuntime)               \
    X(kNemoRt6x4, double, 4, kFbSlots, LensRuntime)               \
    X(kNemoRt10x4, double, 4, kBlmSlots, LensRuntime)             \
    X(kNemo128F32, float, 12, kBlmSlots, LensSlaney128)           \
    X(kNemo80F32, float, 12, kFbSlots, LensSlaney80)

using FbankNemoStreamKernel = void (*)(const FbankNemoStreamParams);
// the stream form of a batch kernel (nullptr: it has none)  (fbank512_nemo_stream.hip)
FbankNemoStreamKernel nemo_stream_kernel(host::K512 batch_kernel);

struct BlmStreamStatsParams {
    const StreamEntry *entries; // the push: stream, frames, out_off (first float of the entry's [n_mels][frames] rows)
    const float *rows;
    double *moments;            // [n_streams][2][n_mels]: mean, M2
    unsigned long long *counts; // [n_streams]
    int n_mels;
};
struct BlmStreamMomentsParams {
    const uint32_t *ids;        // [n]
    const double *moments;
    const unsigned long long *counts;
    float *mean, *inv_std;      // [n][n_mels]
    uint32_t n;
    int n_mels;
};
constexpr int kBlmStreamStatsThreads = 128;
__global__ void blm_stream_stats_kernel(const BlmStreamStatsParams p);        // fbank512_nemo_stream.hip
__global__ void blm_stream_moments_kernel(const BlmStreamMomentsParams p);

}  // namespace melspec
