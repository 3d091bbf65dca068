// blm_stats_plan.hpp -- the host side of the NeMo frontend's split output (melspec_blm_compute_uniform_device_split and
// melspec_blm_compute_ragged_device_split, fbank512.hip) that is arithmetic only: the checks of the calls' arguments and the plans of their
// batches.  Nothing from HIP in here: tests/cpp/blm_stats_host.cpp and blm_stats_ragged_host.cpp build it on the host, with and without
// sanitizers.
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

// ---- the ragged form (melspec_blm_compute_ragged_device_split) ---------------------------------------------------------------------------
// Clips of any width in one launch.  EVERY clip's unit count is rounded up to a multiple of `waves`, an empty clip's being 0, so that
//   - a round of the workgroup lies inside one clip, and no wave of a round is without a unit: RoundStats::wait_free and
//     StagedRows::wait_staged wait for every wave of the round, and a round with a wave missing would never end;
//   - a clip is cut into the blocks blm_stats_plan cuts it into when it is alone: its partials, and so its statistics, are the same bits;
//   - unit_prefix[c] / waves = block_prefix[c] is the clip's first block among the batch's, and n_units / waves the number of blocks.
struct BlmStatsRaggedPlan {
    uint32_t waves = 0;               // 8: the f64 kernel, 12: the f32 kernel
    uint32_t block_frames = 0;        // waves * 4
    uint32_t n_blocks = 0;            // of the batch: the kernels count them in 32 bits
    uint64_t n_units = 0;             // n_blocks * waves
    uint64_t part_bytes = 0;          // the partials: [n_blocks][n_mels] pairs of floats
};
// plan_ragged's unit count of a clip (aux.hip): ceil(frames / frames_per_unit), rounded up to a multiple of round_units (1: as it is).
// With (cols, 4, waves) this has to be blm_stats_blocks(cols) * waves: tests/cpp/blm_stats_ragged_host.cpp holds the two together.
inline uint64_t ragged_clip_units(uint64_t frames, uint32_t frames_per_unit, uint32_t round_units) {
    const uint64_t units = frames / frames_per_unit + (frames % frames_per_unit != 0);
    return round_units <= 1 ? units : (units / round_units + (units % round_units != 0)) * round_units;
}
// the blocks of a clip of `cols` columns (0: none); what blm_stats_plan calls blocks_per_clip
inline uint64_t blm_stats_blocks(uint64_t cols, uint32_t block_frames) { return cols == 0 ? 0 : (cols - 1) / block_frames + 1; }
// block_prefix: nullptr, or [n_clips + 1] for the exclusive prefix of the clips' blocks (written as far as the plan got).  false: no
// clips, no columns at all, or a batch whose blocks do not fit 32 bits or whose scratch does not fit size_t
inline bool blm_stats_plan_ragged(const uint64_t *cols, uint32_t n_clips, int n_mels, bool f32, BlmStatsRaggedPlan &pl, uint64_t *block_prefix = nullptr) {
    pl = BlmStatsRaggedPlan{};
    pl.waves = f32 ? kBlmStatsWavesF32 : kBlmStatsWavesF64;
    pl.block_frames = pl.waves * kBlmStatsFramesPerUnit;
    if (!cols || n_clips == 0 || n_mels <= 0) return false;
    uint64_t total = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        if (block_prefix) block_prefix[c] = total;
        const uint64_t blocks = blm_stats_blocks(cols[c], pl.block_frames);        // <= 2^64 / 32
        if (blocks > 0xffffffffull - total) return false;
        total += blocks;
    }
    if (block_prefix) block_prefix[n_clips] = total;
    if (total == 0) return false;
    pl.n_blocks = static_cast<uint32_t>(total);
    pl.n_units = total * pl.waves;                                            // < 2^36
    if (total > (static_cast<uint64_t>(SIZE_MAX) - 16) / (static_cast<uint64_t>(n_mels) * 2 * sizeof(float))) return false;
    pl.part_bytes = total * static_cast<uint64_t>(n_mels) * 2 * sizeof(float);
    return true;
}

// The ragged call's arguments, in the order melspec_blm_compute_ragged_device checks its own: the context, what it supports, an empty
// batch, the host tables, a batch without a column (most_cols: the widest clip's columns, which the caller can only know once the
// tables are there -- 0 otherwise), the device pointers.
inline BlmStatsArgs blm_stats_ragged_args(bool have_ctx, bool supported, uint32_t n_clips, const void *h_offsets, const void *h_lengths, uint64_t most_cols,
                                          const void *pcm, const void *rows, const void *mean, const void *inv_std) {
    if (!have_ctx) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "blm is NULL"};
    if (!supported) return {kBlmStatsFail, MELSPEC_ERR_UNSUPPORTED, nullptr};
    if (n_clips == 0) return {kBlmStatsDone, MELSPEC_OK, nullptr};
    if (!h_offsets || !h_lengths) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL"};
    if (most_cols == 0) return {kBlmStatsDone, MELSPEC_OK, nullptr};
    if (!pcm || !rows) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"};
    if (!mean || !inv_std) return {kBlmStatsFail, MELSPEC_ERR_INVALID_ARG, "d_mean / d_inv_std is NULL"};
    return {kBlmStatsGo, MELSPEC_OK, nullptr};
}

}  // namespace host
}  // namespace melspec
