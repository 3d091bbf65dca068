// fbank512_kaldi_io_kernels.hpp -- the Kaldi fbank with the sample type (float, int16_t) and the row type (float, f16, bf16) as template
// parameters: melspec_fbank_compute_*_device_io / melspec_fbank_compute_host_io.
//   fbank512_kaldi_io_kernel: the body of fbank512_wave_kernel's Kaldi flavour in its run-per-wave form (the same text, included again):
//     same grid, same runs, same arithmetic; only the loads of fb_kaldi_input (one 4-byte load per int16 sample pair and a 2-byte load for
//     the sample in front of it, times 2^-15, exact; the sample indices of the f32 kernel) and the store of fb_phase3_store (one 16-bit
//     store per lane and value, the f32 value rounded to nearest even once by the store's conversion) differ.  Like its original it has no
//     wait of one wave on another: no barrier in the unit loop, no counter, no polling.
//   cmn_io_kernel: the CMN with a 16-bit output.  A 16-bit row cannot be normalised in place: the main kernel writes its f32 rows, packed in
//     clip order, into a scratch of the object and this pass reads them there and writes row - mean, rounded once, to the caller's rows:
//     4 + 2 bytes per element instead of 4 + 4.  Its body is cmn_kernel's, the same text included again (fbank512_cmn_body.inc) with
//     kSplit = true.
// Instantiated in a translation unit of their own (fbank512_kaldi_io.hip): a new neighbour in a unit changes the schedule of the kernels
// that are already there.  fbank512_clip_kernel (the workgroup-per-clip form, whose waves wait for each other) has its typed variant in
// fbank512_kaldi_split_io_kernels.hpp, for the split output only: these calls, which subtract, stay on the two kernels here.
#pragma once
#include "fbank512_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

template <class T, int WAVES, int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_kaldi_io_kernel(const FbankFastParams p) {
    constexpr int FLAVOR = kFlavorKaldi;
    constexpr bool RUNS = true;        // what launch_fused512 runs for this flavour at eight waves (frame-major plain output)
#define MS_FB512_IN In
#define MS_FB512_OUT Out
#include "fbank512_wave_body.inc"
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

struct CmnIoParams {
    BatchDesc b;                // the clip geometry; b.out: the f32 rows, packed in clip order (uniform: b.out_stride apart, ragged: at b.d_out_off)
    void *dst;                  // the caller's rows of the kernel's row type
    const uint64_t *d_dst_off;  // ragged batches: the first element of clip c in dst (uniform batches: c * b.out_stride)
    int n_mels;
    int rows_per_chunk;
};
constexpr int kCmnThreads = 512;      // cmn_kernel<512>'s

template <class Out>
__global__ __launch_bounds__(kCmnThreads) void cmn_io_kernel(const CmnIoParams p) {
    constexpr int NT = kCmnThreads;
    constexpr bool kSplit = true;
    Out *const dst = static_cast<Out *>(p.dst);
    const uint64_t *const d_dst_off = p.d_dst_off;
    constexpr float *d_means = nullptr;
#include "fbank512_cmn_body.inc"
}

}  // namespace melspec
