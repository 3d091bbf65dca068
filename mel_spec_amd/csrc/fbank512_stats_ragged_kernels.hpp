// fbank512_stats_ragged_kernels.hpp -- the ragged form of the NeMo / Parakeet frontend's split output
// (melspec_blm_compute_ragged_device_split): clips of any length in one launch, each with the rows, the mean and the 1 / (std + 1e-5) that
// melspec_blm_compute_uniform_device_split gives for that clip alone, bit for bit.
//   fbank512_nemo_stats_ragged_kernel: fbank512_nemo_stats_kernel's text (fbank512_wave_body.inc with MS_FB512_STATS) included once more
//     with MS_FB512_STATS_RAGGED, over the ragged batch of the raw call (mel_major, d_len, d_valid, rows as wide as the clip's columns).
//     The plan rounds EVERY clip's unit count up to a multiple of WAVES (blm_stats_plan_ragged, plan_ragged's round_units), so
//       - a round of the workgroup lies inside one clip and covers WAVES x 4 consecutive frames counted from that clip's first frame: the
//         blocks of a clip are the blocks the uniform call cuts it into, and so are their partials;
//       - no wave of a round is without a unit -- what RoundStats::wait_free and StagedRows::wait_staged wait for always comes;
//       - unit_prefix[clip] / WAVES is the clip's first block among the batch's, and a round's block is its index among the batch's rounds
//         (first / WAVES, which the body counts in sblock): the partials lie at part[that index][mel], no table of their own.
//     A block's valid frames come from d_valid[clip].  The f32 kernel reduces a round while it is in the next one, possibly in another
//     clip: it carries the drained round's count in one scalar register.
//   blm_stats_finish_ragged_kernel: blm_stats_finish_kernel with the clip's first block from the unit prefix and its valid frames from
//     d_valid; same merge order, same single rounding; a clip without a valid frame is skipped (its two slots stay as they were).
// Instantiated in a translation unit of their own (fbank512_stats_ragged.hip): the kernels that exist keep the instructions they have.
#pragma once
#include "fbank512_stats_kernels.hpp"

namespace melspec {

struct FbankStatsRaggedParams {
    FbankFastParams f;          // a ragged feature-major batch whose clips' unit counts are each a multiple of the kernel's waves
    float2 *d_part;             // [rounds of the batch = n_units / WAVES][n_mels] {c = the block's mean, squares around c}
};

template <class T, int WAVES, int NSLOTS, class Lens>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_nemo_stats_ragged_kernel(const FbankStatsRaggedParams q) {
    constexpr int FLAVOR = kFlavorNemo;
    constexpr bool RUNS = false;
    const FbankFastParams &p = q.f;
#define MS_FB512_IN float
#define MS_FB512_OUT float
#define MS_FB512_STATS 1
#define MS_FB512_STATS_RAGGED 1
#include "fbank512_wave_body.inc"
#undef MS_FB512_STATS_RAGGED
#undef MS_FB512_STATS
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

struct BlmStatsFinishRaggedParams {
    const float2 *part;             // [blocks of the batch][n_mels]
    float *mean, *inv_std;          // [n_clips][n_mels]
    const uint64_t *d_valid;        // [n_clips]: valid frames (0: the clip has no statistics)
    const uint64_t *d_unit_prefix;  // [n_clips + 1]: the plan's, every entry a multiple of `waves`
    uint32_t n_clips, waves, block_frames;
    int n_mels;
};
__global__ void blm_stats_finish_ragged_kernel(const BlmStatsFinishRaggedParams p);       // fbank512_stats_ragged.hip

}  // namespace melspec
