// blm_split_io_plan.hpp -- the host side of the NeMo frontend's split output with 16-bit ends (melspec_blm_compute_*_split_io, fbank512.hip)
// that is arithmetic only: the dtype codes, the checks of the calls' arguments in the order of the f32 split calls (blm_stats_plan.hpp)
// with the two checks of the _io calls added where those calls have them, and the index of a kernel in the side tables of
// fbank512_stats_io.hip / fbank512_stats_ragged_io.hip.  The plans are the f32 split calls' own (blm_stats_plan, blm_stats_plan_ragged):
// they count elements.  Nothing from HIP in here: tests/cpp/blm_split_io_host.cpp builds it on the host, with and without sanitizers.
#pragma once
#include "blm_stats_plan.hpp"
#include "fused512_route.hpp"

namespace melspec {
namespace host {

// ---- the side tables: [stats kernel of the f32 split call][io_index of the (sample, row) combination] -----------------------------------
constexpr int kBlmSplitIoCombos = 5;                                                                           // MS_IO_COMBOS: every pair but (F32, F32)
constexpr int kBlmSplitIoStatsKernels = static_cast<int>(K512::kAuto80Vote) - static_cast<int>(K512::kStats128);    // MS_K512_STATS
constexpr int kBlmSplitIoKernels = kBlmSplitIoStatsKernels * kBlmSplitIoCombos;
// < 0: `stats` is not a stats kernel, or io is (F32, F32) -- the existing kernels' -- or not a combination at all
constexpr int blm_split_io_slot(K512 stats, int io) {
    return !is_stats(stats) || io_index(io) < 0 ? -1 : (static_cast<int>(stats) - static_cast<int>(K512::kStats128)) * kBlmSplitIoCombos + io_index(io);
}

// ---- the arguments ------------------------------------------------------------------------------------------------------------------------
constexpr bool blm_split_io_pcm_known(int t) { return t == MELSPEC_PCM_F32 || t == MELSPEC_PCM_S16; }
constexpr bool blm_split_io_out_known(int t) { return t == MELSPEC_OUT_F32 || t == MELSPEC_OUT_F16 || t == MELSPEC_OUT_BF16; }
constexpr size_t blm_split_io_pcm_bytes(int t) { return t == MELSPEC_PCM_S16 ? 2 : 4; }
constexpr size_t blm_split_io_out_bytes(int t) { return t == MELSPEC_OUT_F32 ? 4 : 2; }
inline bool blm_split_io_misaligned(const void *pcm, int pcm_dtype, const void *rows, int out_dtype) {
    return (reinterpret_cast<uintptr_t>(pcm) & (blm_split_io_pcm_bytes(pcm_dtype) - 1)) || (reinterpret_cast<uintptr_t>(rows) & (blm_split_io_out_bytes(out_dtype) - 1));
}

// The context and the dtype codes, as the _io calls check them: in front of everything else.  kBlmStatsGo: io = pcm_dtype | out_dtype << 4
// (0: (F32, F32), which the caller hands to the f32 split call as it is).
inline BlmStatsArgs blm_split_io_codes(bool have_ctx, int pcm_dtype, int out_dtype, int &io) {
    io = 0;
    if (!have_ctx) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "blm is NULL"};
    if (!blm_split_io_pcm_known(pcm_dtype)) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16"};
    if (!blm_split_io_out_known(out_dtype)) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "out_dtype must be MELSPEC_OUT_F32, MELSPEC_OUT_F16 or MELSPEC_OUT_BF16"};
    io = pcm_dtype | out_dtype << 4;
    return {kBlmStatsGo, MELSPEC_OK, nullptr};
}
// Behind that the f32 split call's checks in its order, and the alignment of the two typed pointers behind the NULL checks (where
// blm_uniform / blm_ragged have it).  io: a valid combination.
inline BlmStatsArgs blm_split_io_args(bool supported, uint32_t n_clips, uint64_t cols, const void *pcm, const void *rows, const void *mean, const void *inv_std, int io) {
    const BlmStatsArgs a = blm_stats_args(true, supported, n_clips, cols, pcm, rows, mean, inv_std);
    if (a.verdict != kBlmStatsGo) return a;
    if (blm_split_io_misaligned(pcm, io & 15, rows, io >> 4)) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type"};
    return a;
}
inline BlmStatsArgs blm_split_io_ragged_args(bool supported, uint32_t n_clips, const void *h_offsets, const void *h_lengths, uint64_t most_cols, const void *pcm,
                                             const void *rows, const void *mean, const void *inv_std, int io) {
    const BlmStatsArgs a = blm_stats_ragged_args(true, supported, n_clips, h_offsets, h_lengths, most_cols, pcm, rows, mean, inv_std);
    if (a.verdict != kBlmStatsGo) return a;
    if (blm_split_io_misaligned(pcm, io & 15, rows, io >> 4)) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type"};
    return a;
}

}  // namespace host
}  // namespace melspec
