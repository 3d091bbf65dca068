// fbank512_io_kernels.hpp -- the NeMo / Parakeet frontend with the sample type (float, int16_t) and the row type (float, f16, bf16) as
// template parameters: melspec_blm_compute_*_device_io / melspec_blm_compute_host_io.
//   fbank512_nemo_io_kernel: the body of fbank512_wave_kernel's NeMo flavour (the same text, included again): same grid, same rounds,
//     same arithmetic; only the load of nemo_column (one 4-byte load per int16 sample pair and a 2-byte load for the sample in front of
//     it, times 2^-15, exact) and the store (nemo_phase3_store: one 16-bit store per lane and value; StagedRows::drain: 8 bytes per
//     piece of four columns) differ.  The f32 value is rounded to nearest even once, by the store's conversion.
//   blm_normalize_io_kernel / blm_normalize_ragged_io_kernel: normalize_per_feature with a 16-bit output.  A 16-bit row cannot be
//     normalised in place: the main kernel writes its f32 rows (pad columns included) into a scratch of the context and these passes read
//     the rows from there and write (v - mean) / sd, rounded once, and the zero pad columns to the caller's rows: 4 + 2 bytes per element
//     instead of 4 + 4.  Their bodies are those of blm_normalize_kernel / blm_normalize_ragged_kernel, the same text included again
//     (fbank512_norm_body.inc, fbank512_norm_ragged_body.inc) with kSplit = true.
// Instantiated in a translation unit of their own (fbank512_io.hip): a new neighbour in a unit changes the schedule of the kernels that
// are already there.
#pragma once
#include "fbank512_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

template <class T, int WAVES, int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_nemo_io_kernel(const FbankFastParams p) {
    constexpr int FLAVOR = kFlavorNemo;
    constexpr bool RUNS = false;
#define MS_FB512_IN In
#define MS_FB512_OUT Out
#include "fbank512_wave_body.inc"
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

struct BlmNormIoParams {
    const float *src;       // the f32 rows: [n_clips][n_mels][row_w], clips and rows contiguous
    void *dst;              // the caller's rows of the kernel's row type, same shape
    uint64_t row_w;         // columns per row (padded frames)
    uint64_t valid;         // valid frames
    uint32_t n_clips;
    int n_mels;
    int rows_per_group;     // rows staged per workgroup round (<= 64), 0: rows too long for LDS
    int lds_stride;         // floats between staged rows (BlmNormParams::lds_stride)
    // ragged batches (rows_per_group == 0 form only): per clip the first f32 element of the source, the first element of the destination,
    // the row width and the valid frames
    const uint64_t *d_src_off, *d_dst_off, *d_cols, *d_valid;
};

template <class Out>
__global__ __launch_bounds__(kBlmNormThreads) MS_NORM_OCCUPANCY void blm_normalize_io_kernel(const BlmNormIoParams p) {
    constexpr bool kSplit = true;
    const float *const src = p.src;
    Out *const dst = static_cast<Out *>(p.dst);
    const uint64_t *const d_src_off = p.d_src_off, *const d_dst_off = p.d_dst_off;
    const uint64_t clip_stride = p.n_mels * p.row_w;
    constexpr int fold_sel = -1, lab_skip = 0;
    constexpr uint64_t *dbg = nullptr;
#include "fbank512_norm_body.inc"
}

struct BlmNormRaggedIoParams {
    const float *src;
    void *dst;
    const uint64_t *d_src_off, *d_dst_off, *d_cols, *d_valid;   // per clip
    uint32_t n_clips;
    int n_mels;
    int rows_per_group, lds_stride;
    unsigned *ctr;          // zero at launch
};

template <class Out>
__global__ __launch_bounds__(kBlmNormThreads) MS_NORM_OCCUPANCY void blm_normalize_ragged_io_kernel(const BlmNormRaggedIoParams p) {
    constexpr bool kSplit = true;
    const float *const src = p.src;
    Out *const dst = static_cast<Out *>(p.dst);
    const uint64_t *const d_src_off = p.d_src_off, *const d_dst_off = p.d_dst_off;
#include "fbank512_norm_ragged_body.inc"
}

}  // namespace melspec
