// fbank512_stats_io_kernels.hpp -- the NeMo / Parakeet frontend's split output with the sample type (float, int16_t) and the row type
// (float, f16, bf16) as template parameters: melspec_blm_compute_{uniform,ragged}_device_split_io / melspec_blm_compute_host_split_io.
//   fbank512_nemo_stats_io_kernel: the text of fbank512_nemo_stats_ragged_kernel (fbank512_wave_body.inc with MS_FB512_STATS and
//     MS_FB512_STATS_RAGGED) included once more with MS_FB512_IN = In and MS_FB512_OUT = Out: the 16-bit ends of fbank512_nemo_io_kernel and
//     the partials of the split output are independent halves of that text.  Same grid, same rounds, same plans, same LDS.  The
//     partials are taken from the f32 values in front of the store's rounding (f64 kernel: vals[]; f32 kernel: the StagedRows image,
//     which is f32 whatever Out is), so mean and 1 / std are the f32 split call's bits and the rows are its rows rounded to nearest even
//     once.  No scratch rows, no second pass over the rows.
//     ONE kernel for the uniform and the ragged call.  What the ragged text does differently from the uniform one -- a round's partials
//     at [round of the batch] = first / WAVES, the drained round's valid frames carried in a scalar -- holds for a uniform batch planned by
//     blm_stats_plan as well: its clips have blocks_per_clip whole rounds each, so first / WAVES IS clip * blocks_per_clip + block, and the
//     body's locate_unit reads either kind of BatchDesc.  The uniform text's division by blocks_per_clip keeps a reciprocal in a VGPR,
//     which these kernels do not have (the twelve-wave ones spilled it); two copies of the same instructions were not worth a second unit.
//     With MS_FB512_FRESH_FL (the body says what it does): no instantiation uses scratch.
//   blm_stats_finish_kernel / blm_stats_finish_ragged_kernel are reused as they are.
// Instantiated in a translation unit of its own (fbank512_stats_io.hip): the kernels that exist keep the instructions they have.
#pragma once
#include "fused512_route.hpp"
#include "fbank512_stats_ragged_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

// nemo_store_vals with the row type of the 16-bit ends: the f32 value is rounded to nearest even once, by the store's conversion.
// Declared in front of the kernel below: a pointer to a built-in type brings no namespace into the call's lookup.
template <int NSLOTS, class Out>
MS_DEV void nemo_store_vals(int fl, int j, bool store, int n_mels, const float (&vals)[NSLOTS], Out *out_col /* &out[0][first frame of the tile] */, long long row_w) {
    if (!store || j >= kFbOwn) return;
    Out *o = out_col + static_cast<long long>(j) * row_w + fl;
#pragma unroll
    for (int i = 0; i < NSLOTS; ++i)
        if (j + kFbOwn * i < n_mels) o[static_cast<long long>(kFbOwn * i) * row_w] = row_value<Out>(vals[i]);
}

// q.f: a batch whose clips' unit counts are each a multiple of WAVES -- uniform (blm_stats_plan) or ragged (blm_stats_plan_ragged);
// q.d_part: [rounds of the batch = n_units / WAVES][n_mels]
template <class T, int WAVES, int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_nemo_stats_io_kernel(const FbankStatsRaggedParams q) {
    constexpr int FLAVOR = kFlavorNemo;
    constexpr bool RUNS = false;
    const FbankFastParams &p = q.f;
#define MS_FB512_IN In
#define MS_FB512_OUT Out
#define MS_FB512_STATS 1
#define MS_FB512_STATS_RAGGED 1
#define MS_FB512_FRESH_FL 1
#include "fbank512_wave_body.inc"
#undef MS_FB512_FRESH_FL
#undef MS_FB512_STATS_RAGGED
#undef MS_FB512_STATS
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

// The side table: the kernel of a (sample, row) combination for the stats kernel `stats` (K512::kStats128 ..) the f32 split call of the
// context runs on -- same launch shape, same LDS -- and io = pcm_dtype | out_dtype << 4, at [stats][io_index(io)] (blm_split_io_slot,
// blm_split_io_plan.hpp); nullptr: no such kernel.  Defined beside the instantiations (fbank512_stats_io.hip).
using FbankStatsIoKernel = void (*)(const FbankStatsRaggedParams);
FbankStatsIoKernel nemo_stats_io_kernel(host::K512 stats, int io);

}  // namespace melspec
