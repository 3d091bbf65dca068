// whisper_centered_kernels.hpp -- the kernels of the centred Whisper features (melspec_whisper_*; whisper_centered.hip launches them,
// whisper_centered_plan.hpp has the rules):
//   whisper400_six_runs_raw_kernel / whisper400_six64_raw_kernel   the six-frame run kernels (the same text, included again with
//       MS_SIX_RUNS_RAW / MS_SIX64_RAW) without frame maximum, clamp and guard: they store the raw rows log10(max(E, 1e-10)) and fold the
//       maximum of every clip into one word per clip
// and the small kernels, templates over the call's sample / output type (float: whisper_centered.hip; int16, f16, bf16 -- the
// melspec_whisper_*_io calls -- whisper_centered_io.hip, with the typed raw kernels of whisper_centered_io_kernels.hpp)
//   wc_prepare_kernel<In>    sets the clips' maximum words to the floor and gathers the samples of the edge frames (reflection, zeros
//                            beyond the clip) into 400-sample f32 "clips" of one frame each, which the f64 raw kernel then computes like any other
//   wc_fill_kernel<Out>      the silent frames of the split output: rows of -10
//   wc_finalize_kernel<Out>  (max(raw, g - 8) + 4) / 4 of the f32 raw rows, frame-major or mel-major through an LDS tile
// and, in whisper_centered.hip itself,
//   wc_clip_max_kernel       the split output's maxima: biased bits -> float
// The maximum words hold the BIASED value of whisper_six.hpp's phase 3 (log10 + 16, in [6, ~30]): positive floats order like their bit
// patterns, so the per-lane maximum, the wave reduction and the atomic are integer ones.
#pragma once
#include "whisper400_kernels.hpp"
#include "whisper_centered_plan.hpp"

namespace melspec {

constexpr int kWcFloorBits = 0x40C00000;      // 6.0f = -10 + 16

// the raw epilogue of a unit: lane j of a frame stores its values, biased - 16, and keeps the largest biased value it has seen.
// Out: the row type (float; f16 / bf16 in the *_raw_io_* kernels of whisper_centered_io_kernels.hpp): the f32 value rounded to nearest even,
// one store per lane and value as in six_phase4; the maximum is folded from the f32 bits whatever Out is.
template <int NSLOTS, class Out>
__device__ __forceinline__ void six_raw_store(int fl, int j, bool act, int n_mels, const float (&vals)[NSLOTS], Out *out_tile, int &rmax) {
    if (!act || j >= kSixOwn) return;
    Out *o = out_tile + static_cast<long long>(fl) * n_mels + j;
#pragma unroll
    for (int i = 0; i < NSLOTS; ++i) {
        if (j + kSixOwn * i < n_mels) {
            o[i * kSixOwn] = row_value<Out>(vals[i] - 16.0f);
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

// ---- the small kernels ------------------------------------------------------------------------------------------------------------------
// In / Out: the call's sample and row types (float: instantiated in whisper_centered.hip; int16 in, f16 / bf16 out: whisper_centered_io.hip).
// blocks [0, n_edges): the 400 samples of edge frame e to edge_pcm + 400 e (host::wc_source_index's rule; an int16 sample times 2^-15,
// exact -- edge_pcm is f32 whatever In is); the blocks behind them: the maximum words.  No sample at or past n_eff is read.
template <class In>
__global__ __launch_bounds__(256) void wc_prepare_kernel(const In *pcm, const host::WcEdge *edges, uint32_t n_edges, float *edge_pcm, int *slots, uint32_t n_slots) {
    if (blockIdx.x >= n_edges) {
        const uint64_t i = static_cast<uint64_t>(blockIdx.x - n_edges) * 256 + threadIdx.x;
        if (i < n_slots) slots[i] = kWcFloorBits;
        return;
    }
    const host::WcEdge e = edges[blockIdx.x];
    const In *src = pcm + e.pcm_off;
    float *dst = edge_pcm + static_cast<uint64_t>(blockIdx.x) * host::kWcFft;
    for (unsigned i = threadIdx.x; i < host::kWcFft; i += 256) {
        long long idx = static_cast<long long>(e.t * host::kWcHop + i) - static_cast<long long>(host::kWcPad);
        if (idx < 0) idx = -idx;
        if (idx >= static_cast<long long>(e.P)) idx = 2 * (static_cast<long long>(e.P) - 1) - idx;
        dst[i] = idx < static_cast<long long>(e.n_eff) ? pcm_value(src[idx]) : 0.0f;
    }
}

constexpr int kWcTile = 64;      // frames per tile of the fill and finalise passes

// rows [first_silent, T) of every clip: -10 (exact in f16 and bf16).  Grid (clips, tiles of kWcTile frames).  One store per element: a clip's
// rows may start at an odd 16-bit element.
template <class Out>
__global__ __launch_bounds__(256) void wc_fill_kernel(const host::WcRecord *rec, Out *rows, int n_mels) {
    const host::WcRecord r = rec[blockIdx.x];
    const uint64_t tiles = (r.T + kWcTile - 1) / kWcTile;
    for (uint64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint64_t t0 = tile * kWcTile, t1 = t0 + kWcTile < r.T ? t0 + kWcTile : r.T;
        const uint64_t a = (t0 > r.first_silent ? t0 : r.first_silent) * n_mels, b = t1 * n_mels;
        Out *o = rows + r.rows_off;
        for (uint64_t i = a + threadIdx.x; i < b; i += 256) o[i] = static_cast<Out>(host::kWcFloorLog);
    }
}

__device__ __forceinline__ float wc_norm(float raw, float lo) { return (__builtin_fmaxf(raw, lo) + 4.0f) * 0.25f; }

// One tile of kWcTile frames x n_mels per pass; the raw rows are f32 whatever Out is, the clamp runs in f32 and the value is rounded once,
// at the store.  Frame-major: element by element, coalesced.  Mel-major: the tile goes through LDS ([mel][kWcTile + 1] floats: the column
// reads of the transpose hit 32 different banks) and leaves as row pieces of kWcTile values -- 16-byte stores of 16 / sizeof(Out) values
// where the clip's rows allow it (host::wc_wide_ok: T and the clip's first element multiples of four floats / eight 16-bit values, d_out
// 16-byte aligned: WHISPER's 3000-frame clips always), single elements otherwise.  Silent frames are not read: their value is a function
// of the clip maximum alone.  Grid (clips, tiles).  LDS: n_mels * (kWcTile + 1) floats (mel-major only).
template <class Out>
__global__ __launch_bounds__(256) void wc_finalize_kernel(const host::WcRecord *rec, const float *rows, const int *slots, Out *out, int n_mels, int mel_major) {
    extern __shared__ __attribute__((aligned(16))) float wc_tile[];
    constexpr int kVec = 16 / sizeof(Out);
    struct alignas(16) Piece { Out v[kVec]; };
    const host::WcRecord r = rec[blockIdx.x];
    const float lo = (six_float(slots[blockIdx.x]) - 16.0f) - 8.0f;
    const float silent = wc_norm(host::kWcFloorLog, lo);
    const uint64_t tiles = (r.T + kWcTile - 1) / kWcTile;
    const float *in = rows + r.rows_off;
    Out *o = out + r.out_off;
    const int tid = threadIdx.x;
    for (uint64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        const uint64_t t0 = tile * kWcTile;
        const int nt = static_cast<int>(r.T - t0 < static_cast<uint64_t>(kWcTile) ? r.T - t0 : kWcTile);
        const int live = r.first_silent <= t0 ? 0 : static_cast<int>(r.first_silent - t0 < static_cast<uint64_t>(nt) ? r.first_silent - t0 : nt);      // frames of the tile with rows
        const int n = nt * n_mels, nl = live * n_mels;
        if (!mel_major) {
            for (int i = tid; i < n; i += 256) o[t0 * n_mels + i] = row_value<Out>(i < nl ? wc_norm(in[t0 * n_mels + i], lo) : silent);
            continue;
        }
        constexpr int kStride = kWcTile + 1;
        for (int i = tid; i < nl; i += 256) {
            const int t = i / n_mels, m = i - t * n_mels;
            wc_tile[m * kStride + t] = wc_norm(in[t0 * n_mels + i], lo);
        }
        __syncthreads();
        const bool wide = nt == kWcTile && host::wc_wide_ok(r.T, r.out_off, reinterpret_cast<uintptr_t>(out), sizeof(Out));
        if (wide) {
            for (int i = tid; i < n_mels * (kWcTile / kVec); i += 256) {
                const int m = i / (kWcTile / kVec), q = i - m * (kWcTile / kVec);
                const float *s = wc_tile + m * kStride + kVec * q;
                Piece v;
#pragma unroll
                for (int k = 0; k < kVec; ++k) v.v[k] = row_value<Out>(kVec * q + k < live ? s[k] : silent);
                *reinterpret_cast<Piece *>(o + static_cast<uint64_t>(m) * r.T + t0 + kVec * q) = v;
            }
        } else {
            for (int i = tid; i < n_mels * kWcTile; i += 256) {
                const int m = i / kWcTile, t = i - m * kWcTile;
                if (t < nt) o[static_cast<uint64_t>(m) * r.T + t0 + t] = row_value<Out>(t < live ? wc_tile[m * kStride + t] : silent);
            }
        }
        __syncthreads();
    }
}

}  // namespace melspec
