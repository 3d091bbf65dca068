// fbank512_stats_kernels.hpp -- the NeMo / Parakeet frontend's split output (melspec_blm_compute_uniform_device_split): the un-normalised
// log-mel rows plus, per (clip, mel) row, the mean and 1 / (std + 1e-5) of normalize_per_feature (src/mel.rs:721-749), without a second
// pass over the rows.  (Inside this family "split" already names the 16-bit normalisers' kSplit; everything here is called "stats".)
//   fbank512_nemo_stats_kernel: the body of fbank512_wave_kernel's NeMo flavour (the same text, included again with MS_FB512_STATS): same
//     arithmetic and the same stores, so the rows are the bits of the raw call.  The batch is planned with every clip's unit count rounded
//     up to a multiple of WAVES (blm_stats_plan.hpp; the units past the row's width compute and store nothing), so a round of the
//     workgroup lies inside one clip and covers a BLOCK of WAVES x 4 consecutive frames counted from the clip's first frame.  Per round
//     and mel row the workgroup leaves one partial {c, sum of the squared distances of the block's valid values from c} at
//     part[clip][block][mel] -- plain vector stores, one writer per word, no atomics.  c is the block's mean to within an ulp, built as
//     first value + mean of the distances from it: a constant block (digital silence) gives c = that constant and squares of exactly 0,
//     where a plain f32 sum of 48 equal values already rounds -- and its error would come out of the merge as a standard deviation.
//       f32 (twelve waves): the round's values sit in the StagedRows image; after draining it, sixteen adjacent lanes take a mel row
//         (one 16-byte piece of four columns each, twelve of them) and reduce it over DPP (StagedStats).
//       f64 (eight waves): a wave folds its four frames (lanes fl * 16 + j) with lane swaps into the same pair for its unit, leaves it
//         in LDS, and the wave that arrives last merges the eight units in unit order in f64 (RoundStats).
//   blm_stats_finish_kernel: one thread per (clip, mel) merges the clip's partials in block order in f64 (the pairwise update of Chan et
//     al.: M2 += M2_b + n_b n (mean_b - mean)^2 / (n + n_b)) and rounds once: mean and inv_std = 1 / (sqrt(M2 / max(valid - 1, 1)) + 1e-5).
// What a block holds depends on the clip's samples, its length and the precision mode only -- not on the clip's place in the batch, the
// batch's size, the grid or what ran before (the rule of CmnTree, fbank512_kernels.hpp) -- and so do the statistics, to the last bit.
// Instantiated in a translation unit of their own (fbank512_stats.hip): the kernels that exist keep the instructions they have.
#pragma once
#include "fbank512_kernels.hpp"

namespace melspec {

struct FbankStatsParams {
    FbankFastParams f;          // a uniform batch whose units_per_clip is a multiple of the kernel's waves
    float2 *d_part;             // [n_clips][blocks_per_clip][n_mels] {c = the block's mean, squares around c}
    uint32_t blocks_per_clip;   // units_per_clip / WAVES
};

// nemo_phase3_store's stores for values that are already computed (vals: this lane's mel j + 15 i of frame fl, zero for a column past the
// valid frames)
template <int NSLOTS>
MS_DEV void nemo_store_vals(int fl, int j, bool store, int n_mels, const float (&vals)[NSLOTS], float *out_col /* &out[0][first frame of the tile] */, long long row_w) {
    if (!store || j >= kFbOwn) return;
    float *o = out_col + static_cast<long long>(j) * row_w + fl;
#pragma unroll
    for (int i = 0; i < NSLOTS; ++i)
        if (j + kFbOwn * i < n_mels) o[static_cast<long long>(kFbOwn * i) * row_w] = vals[i];
}

// the sum over the wave's four rows of sixteen lanes (one frame each), the same bits in every lane: (row 0 + row 1) + (row 2 + row 3).
// Both operands of a swap are the same register, so whichever half the instruction moves, the two results are the two addends.
MS_DEV float stats_sum_frames(float v) {
    const unsigned x = __builtin_bit_cast(unsigned, v);
    const auto a = __builtin_amdgcn_permlane16_swap(x, x, false, false);         // rows 1, 3 of one copy <-> rows 0, 2 of the other
    const float t = __builtin_bit_cast(float, static_cast<unsigned>(a[0])) + __builtin_bit_cast(float, static_cast<unsigned>(a[1]));
    const unsigned y = __builtin_bit_cast(unsigned, t);
    const auto b = __builtin_amdgcn_permlane32_swap(y, y, false, false);         // lanes 32-63 of one copy <-> lanes 0-31 of the other
    return __builtin_bit_cast(float, static_cast<unsigned>(b[0])) + __builtin_bit_cast(float, static_cast<unsigned>(b[1]));
}

template <int CTRL>
MS_DEV float stats_dpp(float x) {
    const int i = __builtin_bit_cast(int, x);
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(i, i, CTRL, 0xf, 0xf, true));
}
// the sum over a row of sixteen lanes, the same bits in every lane: a butterfly of DPP exchanges
MS_DEV float stats_sum_row16(float v) {
    v += stats_dpp<0xB1>(v);       // quad_perm [1, 0, 3, 2]
    v += stats_dpp<0x4E>(v);       // quad_perm [2, 3, 0, 1]
    v += stats_dpp<0x141>(v);      // row_half_mirror
    v += stats_dpp<0x140>(v);      // row_mirror
    return v;
}

// f32 kernel: the partials of a drained round from its StagedRows image.  Every wave of a round is in the same block, so a wave knows
// the block it is draining (dst, n) from its own previous round.
template <int WAVES>
struct StagedStats {
    // all threads; tid: opaque to the optimiser like StagedRows::drain's.  dst = &part[clip][block][0], n = the block's valid frames.
    // Written to hold little across the rows' loop (one lane-dependent value, kk): this step sits where the twelve-wave kernel keeps all
    // its loop invariants, with two registers to spare.
    template <class Staged>
    __device__ __forceinline__ static void reduce(const Staged &st, unsigned r, int tid, float2 *dst, int n) {
        static_assert(Staged::kCols == WAVES * kFbFPW && WAVES <= 16, "sixteen lanes per mel row, a unit's four columns each");
        const float inv_n = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, f32_div_rn(1.0f, static_cast<float>(n > 0 ? n : 1)))));
        const float *img = st.image + (r & 1u) * Staged::image_floats(st.n_mels);
        const int kk = n - ((tid & 15) << 2);          // this lane's columns k = 0 .. 3 are valid frames for k < kk (n <= 4 * WAVES: none for lanes >= WAVES)
#pragma unroll 1
        for (int m0 = 0; m0 < st.n_mels; m0 += WAVES * 4) {          // workgroup-uniform trip count: every lane takes part in the exchanges
            const int m = m0 + (tid >> 4);
            f4 v = ld4(img + (m < st.n_mels ? m : 0) * Staged::kPitch + ((tid & 15) < WAVES ? (tid & 15) << 2 : 0));
            const float first = stats_sum_row16(kk == n ? v.x : 0.0f);                          // the block's first value, held by the row's lane 0
            v.x = kk > 0 ? v.x - first : 0.0f; v.y = kk > 1 ? v.y - first : 0.0f; v.z = kk > 2 ? v.z - first : 0.0f; v.w = kk > 3 ? v.w - first : 0.0f;
            const float shift = f32_mul_rn(stats_sum_row16((v.x + v.y) + (v.z + v.w)), inv_n);
            v.x = kk > 0 ? v.x - shift : 0.0f; v.y = kk > 1 ? v.y - shift : 0.0f; v.z = kk > 2 ? v.z - shift : 0.0f; v.w = kk > 3 ? v.w - shift : 0.0f;
            const float q = stats_sum_row16((f32_mul_rn(v.x, v.x) + f32_mul_rn(v.y, v.y)) + (f32_mul_rn(v.z, v.z) + f32_mul_rn(v.w, v.w)));
            if (m < st.n_mels && kk == n) dst[m] = make_float2(first + shift, q);
        }
    }
};

// {mean, squares around it} of a set of n values (n == 0: the empty start) merged with those of nb > 0 more, in f64
__device__ __forceinline__ void stats_merge(double &mean, double &M2, double &n, double mean_b, double m2b, double nb) {
    if (n == 0.0) { mean = mean_b; M2 = m2b; n = nb; return; }
    const double delta = mean_b - mean, tot = n + nb;
    M2 += m2b + delta * delta * (n * nb / tot);
    mean += delta * (nb / tot);
    n = tot;
}

// f64 kernel: one buffer of the waves' unit partials [WAVES][n_mels] and two counters; the wave that arrives last merges, a wave puts the
// next round's partial there only after that merge (a split barrier with a round of slack: a wave arrives at the end of round r and waits
// in front of its put of round r + 1)
template <int WAVES>
struct RoundStats {
    float2 *part;            // [WAVES][n_mels]
    unsigned *arrived, *freed;
    int n_mels;
    unsigned round = 0;
    __device__ __forceinline__ RoundStats(void *base, unsigned *counters, int mels) : part(static_cast<float2 *>(base)), arrived(counters), freed(counters + 1), n_mels(mels) {}
    static constexpr size_t bytes(int n_mels) { return static_cast<size_t>(WAVES) * n_mels * sizeof(float2); }
    __device__ __forceinline__ void wait_free(int lane) const {
        // (like StagedRows::wait_staged: every wave of the workgroup arrives in every round, so the merge it waits for always comes)
        if (lane == 0)
            while (__hip_atomic_load(freed, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < round) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_wave_barrier();
    }
    // every lane, behind the wave's writes to part[wave]: dst = &part of the block in global memory, nb = the block's valid frames
    __device__ __forceinline__ void arrive(int lane, float2 *dst, int nb) {
        __builtin_amdgcn_wave_barrier();
        unsigned old = 0;
        if (lane == 0) old = __hip_atomic_fetch_add(arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_ballot_w64(lane == 0 && old == (round + 1) * WAVES - 1) != 0) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
            for (int m = lane; m < n_mels; m += 64) {
                // the units in order; the units in front of unit w are full, so its weight nb / (4 w + nb) is a function of (w, nb) alone:
                // one f32 division per unit, the same for every row, instead of stats_merge's two f64 divisions per unit and row -- this
                // merge is what the other waves' next round waits for
                double mean = 0.0, M2 = 0.0, n = 0.0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) {
                    const int left = nb - w * kFbFPW;
                    const float2 u = part[w * n_mels + m];
                    if (left > 0) {
                        const int nw = left < kFbFPW ? left : kFbFPW;
                        if (w == 0) {
                            mean = static_cast<double>(u.x); M2 = static_cast<double>(u.y);
                        } else {
                            const double r = static_cast<double>(f32_div_rn(static_cast<float>(nw), static_cast<float>(w * kFbFPW + nw)));
                            const double delta = static_cast<double>(u.x) - mean;
                            M2 += static_cast<double>(u.y) + delta * delta * (static_cast<double>(w * kFbFPW) * r);
                            mean += delta * r;
                        }
                        n = static_cast<double>(w * kFbFPW + nw);
                    }
                }
                // c rounds the block's mean once; the squares are moved to c: sum (x - c)^2 = M2 + n (mean - c)^2
                const float c = static_cast<float>(mean);
                const double e = mean - static_cast<double>(c);
                dst[m] = make_float2(c, static_cast<float>(M2 + n * e * e));
            }
            __builtin_amdgcn_wave_barrier();
            if (lane == 0) __hip_atomic_store(freed, round + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        ++round;
    }
};

template <class T, int WAVES, int NSLOTS, class Lens>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_nemo_stats_kernel(const FbankStatsParams q) {
    constexpr int FLAVOR = kFlavorNemo;
    constexpr bool RUNS = false;
    const FbankFastParams &p = q.f;
#define MS_FB512_IN float
#define MS_FB512_OUT float
#define MS_FB512_STATS 1
#include "fbank512_wave_body.inc"
#undef MS_FB512_STATS
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

struct BlmStatsFinishParams {
    const float2 *part;         // [n_clips][blocks_per_clip][n_mels]
    float *mean, *inv_std;      // [n_clips][n_mels]
    uint64_t valid;             // valid frames per clip (> 0)
    uint32_t n_clips, blocks_per_clip, block_frames;
    int n_mels;
};
constexpr int kBlmStatsFinishThreads = 256;
__global__ void blm_stats_finish_kernel(const BlmStatsFinishParams p);       // fbank512_stats.hip

}  // namespace melspec
