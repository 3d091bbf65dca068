// whisper_centered_kernels.hpp -- the kernels of the centred Whisper features (melspec_whisper_*; whisper_centered.hip launches them,
// whisper_centered_plan.hpp has the rules):
//   whisper400_six_runs_raw_kernel / whisper400_six64_raw_kernel   the six-frame run kernels (the same text, included again with
//       MS_SIX_RUNS_RAW / MS_SIX64_RAW) without frame maximum, clamp and guard: they store the raw rows log10(max(E, 1e-10)) and fold the
//       maximum of every clip into one word per clip
// and, in whisper_centered.hip itself,
//   wc_prepare_kernel      sets the clips' maximum words to the floor and gathers the samples of the edge frames (reflection, zeros
//                          beyond the clip) into 400-sample "clips" of one frame each, which the f64 raw kernel then computes like any other
//   wc_fill_kernel         the silent frames of the split output: rows of -10
//   wc_clip_max_kernel     the split output's maxima: biased bits -> float
//   wc_finalize_kernel     (max(raw, g - 8) + 4) / 4, frame-major or mel-major through an LDS tile
// The maximum words hold the BIASED value of whisper_six.hpp's phase 3 (log10 + 16, in [6, ~30]): positive floats order like their bit
// patterns, so the per-lane maximum, the wave reduction and the atomic are integer ones.
#pragma once
#include "whisper400_kernels.hpp"
#include "whisper_centered_plan.hpp"

namespace melspec {

constexpr int kWcFloorBits = 0x40C00000;      // 6.0f = -10 + 16

// the raw epilogue of a unit: lane j of a frame stores its values, biased - 16, and keeps the largest biased value it has seen
template <int NSLOTS>
__device__ __forceinline__ void six_raw_store(int fl, int j, bool act, int n_mels, const float (&vals)[NSLOTS], float *out_tile, int &rmax) {
    if (!act || j >= kSixOwn) return;
    float *o = out_tile + static_cast<long long>(fl) * n_mels + j;
#pragma unroll
    for (int i = 0; i < NSLOTS; ++i) {
        if (j + kSixOwn * i < n_mels) {
            o[i * kSixOwn] = vals[i] - 16.0f;
            rmax = six_imax(rmax, six_bits(vals[i]));
        }
    }
}
// the wave's run leaves clip `clip` (or ends): one wave reduction, one atomic on the clip's word.  Every lane of the wave calls this.
// Relaxed at agent scope: the word is read by later kernels of the stream only; a maximum does not depend on the order of its operands,
// so the same batch gives the same bits.
__device__ __forceinline__ void six_raw_flush(int *slots, const uint32_t *slot_map, uint32_t clip, int lane, int rmax) {
    const int m = wave_reduce_int<true>(rmax);
    if (lane == 0 && m > 0) {
        const uint32_t s = slot_map ? slot_map[clip] : clip;
        __hip_atomic_fetch_max(slots + s, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct WcRawParams {
    FastParams f;
    int *slots;                  // [clips of the call]: biased maximum bits, kWcFloorBits before the first launch
    const uint32_t *slot_map;    // the word of clip c of THIS launch's batch (the edge launch: its "clips" are frames); nullptr: c
};
struct WcRaw64Params {
    Six64Params f;
    int *slots;
    const uint32_t *slot_map;
};

template <int NSLOTS, class Lens>
__global__ __launch_bounds__(kSixWaves * 64, 4) void whisper400_six_runs_raw_kernel(const WcRawParams q) {
    const FastParams &p = q.f;
    int *const wc_slots = q.slots;
    const uint32_t *const wc_slot_map = q.slot_map;
#define MS_SIX_RUNS_RAW 1
#define MS_SIX_RUNS_WAVES kSixWaves
#define MS_SIX_RUNS_IN float
#define MS_SIX_RUNS_OUT float
#include "whisper400_six_runs_body.inc"
#undef MS_SIX_RUNS_OUT
#undef MS_SIX_RUNS_IN
#undef MS_SIX_RUNS_WAVES
#undef MS_SIX_RUNS_RAW
}

template <int NSLOTS, class Lens>
__global__ __launch_bounds__(kSix64Waves * 64, 3) void whisper400_six64_raw_kernel(const WcRaw64Params q) {
    const Six64Params &p = q.f;
    int *const wc_slots = q.slots;
    const uint32_t *const wc_slot_map = q.slot_map;
#define MS_SIX64_RAW 1
#define MS_SIX64_IN float
#define MS_SIX64_OUT float
#include "whisper400_six64_body.inc"
#undef MS_SIX64_OUT
#undef MS_SIX64_IN
#undef MS_SIX64_RAW
}

}  // namespace melspec
