// stream_banks_io_kernels.hpp -- f16 / bf16 rows out of the Kaldi fbank's and the NeMo / Parakeet frontend's stream banks
// (melspec_fbank_stream_push_*_io, melspec_blm_stream_push_*_io / _finish_*_io).  The running statistics of both banks are folds over the
// f32 rows, and the fold kernels of the f32 pushes read those rows out of the caller's buffer; a 16-bit push has no f32 row there.  As in
// the batch _io calls with CMN (fbank512_kaldi_io_kernels.hpp's cmn_io_kernel) the frame kernel -- the f32 push's, untouched -- writes its
// f32 rows, packed in entry order, into a scratch of the bank, and the pass behind it reads them there:
//   fbank_stream_sum_io_kernel<Out>: fbank_stream_sum_kernel's fold (fbank512_stream.hip), the same operations in the same order, over the
//     scratch; every element it adds it also stores, rounded to nearest even once, at the entry's place in the caller's rows.
//   blm_stream_stats_io_kernel<Out>: blm_stream_stats_kernel's Welford update (fbank512_nemo_stream.hip), likewise and likewise without
//     contraction.
// Each f32 element is read from the scratch once; no kernel reads the caller's rows and there is no conversion pass.  Stores are one 2-byte
// store per element: entries may start at odd elements and share a 4-byte word with a neighbour (in the NeMo layout every mel row of an
// entry with an odd number of columns does), so nothing wider is written.
// The Kaldi twin's lane per bin walks the frames: a wave's loads and stores are the consecutive bins of one frame.  In the NeMo layout the
// lane per mel row walks time, so a wave's accesses are `frames` elements apart.  The first form of the NeMo twin kept that walk for its
// stores as well; at 100 columns per entry (1 s chunks) its push took 1.5 x the f32 push (profiles/stream_banks_io.txt, second table).
// The twin therefore stages the entry through LDS, 64 columns at a time: the workgroup loads [n_mels][64] with consecutive lanes on
// consecutive columns, stores the rounded tile the same way (128 contiguous bytes per mel row), and the lanes fold their rows out of
// LDS.  That push takes 1.02 - 1.07 x the f32 push at 10 ms and 100 ms chunks and 0.97 x at 1 s (the f32 push's fold reads the caller's
// rows `frames` apart).
// Out is f16 or bf16 only: (pcm, MELSPEC_OUT_F32) is the f32 push, on the f32 fold kernels.
// Instantiated in a translation unit of their own (stream_banks_io.hip): the kernels that exist keep the instructions they have.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "stream_plan.hpp"

namespace melspec {

struct FbankStreamSumIoParams {
    const StreamEntry *entries; // the push: stream, frames, out_off (first element of the entry's rows in dst)
    const uint64_t *src_off;    // [n]: first float of the entry's rows in rows (packed in entry order)
    const float *rows;          // the bank's f32 scratch
    void *dst;                  // the caller's rows of the kernel's row type
    double *sums;               // [n_streams][n_mels]
    unsigned long long *counts; // [n_streams]
    int n_mels;
};
struct BlmStreamStatsIoParams {
    const StreamEntry *entries; // the push: stream, frames, out_off (first element of the entry's [n_mels][frames] rows in dst)
    const uint64_t *src_off;    // [n]: first float of the entry's [n_mels][frames] rows in rows (packed in entry order)
    const float *rows;          // the bank's f32 scratch
    void *dst;                  // the caller's rows of the kernel's row type
    double *moments;            // [n_streams][2][n_mels]: mean, M2
    unsigned long long *counts; // [n_streams]
    int n_mels;
    int tile;                   // columns per LDS tile: set by blm_stream_stats_io_launch
};

// one workgroup per entry, queued on s; out_dtype is MELSPEC_OUT_F16 or MELSPEC_OUT_BF16.  Returns hipGetLastError's status.  (stream_banks_io.hip)
hipError_t fbank_stream_sum_io_launch(const FbankStreamSumIoParams &p, int out_dtype, uint32_t n, hipStream_t s);
hipError_t blm_stream_stats_io_launch(const BlmStreamStatsIoParams &p, int out_dtype, uint32_t n, hipStream_t s);

}  // namespace melspec
