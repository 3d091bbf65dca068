// blm_stats_plan.hpp -- the host side of the NeMo frontend's split output (melspec_blm_compute_uniform_device_split, fbank512.hip) that is
// arithmetic only: the checks of the call's arguments and the plan of its batch.  Nothing from HIP in here: tests/cpp/blm_stats_host.cpp
// builds it on the host, with and without sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/melspec_hip.h"

namespace melspec {
namespace host {

constexpr uint32_t kBlmStatsFramesPerUnit = 4;        // kFbFPW
constexpr uint32_t kBlmStatsWavesF64 = 8, kBlmStatsWavesF32 = 12;

// A clip's units are rounded up to whole rounds of the kernel's workgroup (`waves` units of four frames), so that a round lies inside one
// clip and covers a block of waves * 4 consecutive frames counted from the clip's first frame: what a block holds, and with it the
// statistics, depends on the clip alone.
struct BlmStatsPlan {
    uint32_t waves = 0;               // 8: the f64 kernel, 12: the f32 kernel
    uint32_t block_frames = 0;        // waves * 4
    uint32_t units_per_clip = 0;      // a multiple of waves, covering the row's cols columns
    uint32_t blocks_per_clip = 0;     // units_per_clip / waves
    uint64_t n_units = 0;             // units_per_clip * n_clips
    uint64_t part_bytes = 0;          // the partials: [n_clips][blocks_per_clip][n_mels] pairs of floats
};

// false: the batch is larger than the plan's 32-bit unit count per clip or the scratch's size can hold
inline bool blm_stats_plan(uint64_t cols, uint32_t n_clips, int n_mels, bool f32, BlmStatsPlan &pl) {
    pl = BlmStatsPlan{};
    pl.waves = f32 ? kBlmStatsWavesF32 : kBlmStatsWavesF64;
    pl.block_frames = pl.waves * kBlmStatsFramesPerUnit;
    if (cols == 0 || n_clips == 0 || n_mels <= 0) return false;
    const uint64_t blocks = (cols - 1) / pl.block_frames + 1;
    // the kernels count the batch's blocks (clip * blocks_per_clip + block) in 32 bits, the plan a clip's units
    if (blocks > 0xffffffffull / n_clips || blocks > 0xffffffffull / pl.waves) return false;
    pl.blocks_per_clip = static_cast<uint32_t>(blocks);
    pl.units_per_clip = pl.blocks_per_clip * pl.waves;
    pl.n_units = static_cast<uint64_t>(pl.units_per_clip) * n_clips;
    const uint64_t pairs = blocks * n_clips;                              // < 2^32
    pl.part_bytes = pairs * static_cast<uint64_t>(n_mels) * 2 * sizeof(float);
    if (pl.part_bytes > static_cast<uint64_t>(SIZE_MAX) - 16) return false;
    return true;
}

// What the call does with its arguments, in the order the other calls of the context check theirs.  kGo: launch; kDone: MELSPEC_OK with
// nothing written (no clips, or a clip length without a valid frame); otherwise `status` is returned with `msg` as the last error
// (msg == nullptr: the caller words it -- the unsupported context, whose geometry the message names).
enum BlmStatsVerdict { kBlmStatsGo = 0, kBlmStatsDone = 1, kBlmStatsFail = 2 };
struct BlmStatsArgs {
    BlmStatsVerdict verdict;
    int status;
    const char *msg;
};
inline BlmStatsArgs blm_stats_args(bool have_ctx, bool supported, uint32_t n_clips, uint64_t cols, const void *pcm, const void *rows, const void *mean,
                                   const void *inv_std) {
    if (!have_ctx) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "blm is NULL"};
    if (!supported) return {kBlmStatsFail, MELSPEC_ERR_UNSUPPORTED, nullptr};
    if (n_clips == 0 || cols == 0) return {kBlmStatsDone, MELSPEC_OK, nullptr};
    if (!pcm || !rows) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"};
    if (!mean || !inv_std) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "d_mean / d_inv_std is NULL"};
    return {kBlmStatsGo, MELSPEC_OK, nullptr};
}

}  // namespace host
}  // namespace melspec
