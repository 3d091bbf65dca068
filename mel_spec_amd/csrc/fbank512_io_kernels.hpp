// fbank512_io_kernels.hpp -- the NeMo / Parakeet frontend with the sample type (float, int16_t) and the row type (float, f16, bf16) as
// template parameters: melspec_blm_compute_*_device_io / melspec_blm_compute_host_io.
//   fbank512_nemo_io_kernel: the body of fbank512_wave_kernel's NeMo flavour (the same text, included again): same grid, same rounds,
//     same arithmetic; only the load of nemo_column (one 4-byte load per int16 sample pair and a 2-byte load for the sample in front of
//     it, times 2^-15, exact) and the store (nemo_phase3_store: one 16-bit store per lane and value; StagedRows::drain: 8 bytes per
//     piece of four columns) differ.  The f32 value is rounded to nearest even once, by the store's conversion.
//   blm_normalize_io_kernel / blm_normalize_ragged_io_kernel: normalize_per_feature with a 16-bit output.  A 16-bit row cannot be
//     normalised in place: the main kernel writes its f32 rows (pad columns included) into a scratch of the context and these passes read
//     the rows from there -- staging, left-fold mean and variance tree exactly those of blm_normalize_kernel / blm_normalize_ragged_kernel --
//     and write (v - mean) / sd, rounded once, and the zero pad columns to the caller's rows: 4 + 2 bytes per element instead of 4 + 4.
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

// four columns of a row to 16-bit values at dst[0 .. 4) where they lie inside the row (columns [c0, c0 + 4) of row_w): one 8-byte store at
// 2-byte alignment (rows start at odd elements whenever row_w is odd) or element by element at the row's ends
template <class Out>
__device__ __forceinline__ void blm_store4(Out *g, int c0, uint32_t row_w, const float (&o)[4]) {
    if constexpr (sizeof(Out) == 4) {
        typedef float v4u __attribute__((ext_vector_type(4), aligned(4)));
        if (c0 >= 0 && static_cast<uint32_t>(c0 + 3) < row_w) {
            *reinterpret_cast<v4u *>(g) = v4u{o[0], o[1], o[2], o[3]};
            return;
        }
    } else {
        typedef uint32_t w2u __attribute__((ext_vector_type(2), aligned(2)));
        if (c0 >= 0 && static_cast<uint32_t>(c0 + 3) < row_w) {
            const Out h0 = row_value<Out>(o[0]), h1 = row_value<Out>(o[1]), h2 = row_value<Out>(o[2]), h3 = row_value<Out>(o[3]);
            const uint32_t lo = __builtin_bit_cast(uint16_t, h0) | static_cast<uint32_t>(__builtin_bit_cast(uint16_t, h1)) << 16;
            const uint32_t hi = __builtin_bit_cast(uint16_t, h2) | static_cast<uint32_t>(__builtin_bit_cast(uint16_t, h3)) << 16;
            *reinterpret_cast<w2u *>(g) = w2u{lo, hi};
            return;
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (c0 + e >= 0 && static_cast<uint32_t>(c0 + e) < row_w) g[e] = row_value<Out>(o[e]);
}

// KEEP IN STEP with blm_normalize_kernel (fbank512_kernels.hpp): the staging, the mean fold and the sum-of-squares tree are copies of that
// kernel's, operation for operation, and the host sizes both with blm_norm_shape_uniform (fbank512.hip) -- the statistics of a 16-bit call
// are the f32 call's bits only as long as the two agree.  Only the source / destination split and the final store differ.
template <class Out>
__global__ __launch_bounds__(kBlmNormThreads) MS_NORM_OCCUPANCY void blm_normalize_io_kernel(const BlmNormIoParams p) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const uint64_t rows = (uint64_t)p.n_clips * p.n_mels;
    const int tid = threadIdx.x;
    Out *const dst = static_cast<Out *>(p.dst);
    if (p.rows_per_group == 0) {
        for (uint64_t row = (uint64_t)blockIdx.x * kBlmNormThreads + tid; row < rows; row += (uint64_t)gridDim.x * kBlmNormThreads) {
            const float *r;
            Out *d;
            uint64_t valid = p.valid, cols = p.row_w;
            if (p.d_dst_off) {
                const uint64_t clip = row / p.n_mels, m = row - clip * p.n_mels;
                cols = p.d_cols[clip];
                r = p.src + p.d_src_off[clip] + m * cols;
                d = dst + p.d_dst_off[clip] + m * cols;
                valid = p.d_valid[clip];
            } else {
                r = p.src + row * p.row_w;
                d = dst + row * p.row_w;
            }
            if (valid > 0) {
                float mean, sd;
                blm_row_stats_slow(r, valid, mean, sd);
                for (uint64_t k = 0; k < valid; ++k) d[k] = row_value<Out>(f32_div_rn(r[k] - mean, sd));
            }
            for (uint64_t k = valid; k < cols; ++k) d[k] = static_cast<Out>(0.0f);
        }
        return;
    }
    // blm_normalize_kernel's rounds: rows staged whole in LDS from 16-byte granules of the source, at the offset they have in their granule
    const int R = p.rows_per_group, S = p.lds_stride;
    float *stat = tile + (size_t)R * S;      // [R][2]
    constexpr int kRowsAtOnce = 9;
    const uint32_t valid = static_cast<uint32_t>(p.valid);
    const uint32_t src_f = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p.src) >> 2) & 3u;
    const uint32_t nq_max = (valid + 6) / 4;            // granules of a row's valid frames at the worst alignment
    const uint32_t row_w = static_cast<uint32_t>(p.row_w);
    const uint32_t nq_store = (row_w + 6) / 4;          // ... and of the whole row
    const uint64_t per_wg = (rows + gridDim.x - 1) / gridDim.x;
    const uint64_t row_begin = (uint64_t)blockIdx.x * per_wg;
    const uint64_t row_end = row_begin + per_wg < rows ? row_begin + per_wg : rows;
    float *part = stat + 2 * R;              // [R][PP] partial sums of squares
    const int PP = kBlmNormThreads / R;      // threads per row in the variance pass
    for (uint64_t row0 = row_begin; row0 < row_end;) {
        const int nr = row_end - row0 < (uint64_t)R ? (int)(row_end - row0) : R;
        const uint64_t e00 = row0 * p.row_w;
        for (int rr0 = 0; rr0 < nr; rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_max; q += kBlmNormThreads) {
                f4 v[kRowsAtOnce];
                uint32_t to[kRowsAtOnce];
                uint64_t e0 = e00 + (uint64_t)rr0 * p.row_w;
                uint32_t t = static_cast<uint32_t>(rr0) * S;
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {
                    const uint32_t a = (src_f + static_cast<uint32_t>(e0)) & 3u;
                    const uint32_t nq = (a + valid + 3) >> 2;
                    const uint32_t qq = q < nq ? q : nq - 1;
                    v[i] = *reinterpret_cast<const f4 *>(p.src + e0 - a + 4 * qq);
                    to[i] = t + 4 * qq;
                    if (rr0 + i + 1 < nr) { e0 += p.row_w; t += S; }
                }
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) *reinterpret_cast<f4 *>(tile + to[i]) = v[i];
            }
        }
        __syncthreads();
        // the means: the reference's f32 left fold (blm_row_mean_lds), a lane per row
        if (tid < nr) {
            const uint32_t a = (src_f + static_cast<uint32_t>(e00 + (uint64_t)tid * p.row_w)) & 3u;
            MS_PRIO(3);
            stat[2 * tid] = blm_row_mean_lds(tile + (size_t)tid * S, a, valid);
            MS_PRIO(0);
        }
        __syncthreads();
        // the unbiased variance: blm_normalize_kernel's fixed tree
        {
            const int r = tid / PP, pt = tid - r * PP;
            if (r < nr) {
                const uint32_t a = (src_f + static_cast<uint32_t>(e00 + (uint64_t)r * p.row_w)) & 3u;
                const float *row = tile + (size_t)r * S + a;
                const float mean = stat[2 * r];
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                uint32_t k = pt;
                for (; k + 3 * PP < valid; k += 4 * PP) {
                    const float c0 = row[k] - mean, c1 = row[k + PP] - mean, c2 = row[k + 2 * PP] - mean, c3 = row[k + 3 * PP] - mean;
                    a0 += c0 * c0; a1 += c1 * c1; a2 += c2 * c2; a3 += c3 * c3;
                }
                for (; k < valid; k += PP) {
                    const float c = row[k] - mean;
                    a0 += c * c;
                }
                part[r * PP + pt] = (a0 + a1) + (a2 + a3);
            }
        }
        __syncthreads();
        if (tid < nr) {
            const float *pp = part + tid * PP;
            float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
            int i = 0;
            for (; i + 3 < PP; i += 4) { q0 += pp[i]; q1 += pp[i + 1]; q2 += pp[i + 2]; q3 += pp[i + 3]; }
            for (; i < PP; ++i) q0 += pp[i];
            const float q = (q0 + q1) + (q2 + q3);
            float denom = static_cast<float>(valid) - 1.0f;
            denom = denom < 1.0f ? 1.0f : denom;
            const float sd = __builtin_sqrtf(f32_div_rn(q, denom)) + 1e-5f;
            stat[2 * tid + 1] = f32_div_rn(1.0f, sd);
        }
        __syncthreads();
        // every granule of the row goes to the caller: normalised values, then the zero columns up to row_w
        for (int rr0 = 0; rr0 < nr; rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_store; q += kBlmNormThreads) {
                f4 v[kRowsAtOnce];
                float mean[kRowsAtOnce], rsd[kRowsAtOnce];
                const uint32_t ql = q < nq_max ? q : nq_max - 1;          // granules past the staged frames: the last staged one, never used
                uint32_t t = static_cast<uint32_t>(rr0) * S + 4 * ql;
                const float *st = stat + 2 * rr0;
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {           // every LDS read first (rows past the group: its last row again)
                    v[i] = *reinterpret_cast<const f4 *>(tile + t);
                    mean[i] = st[0]; rsd[i] = st[1];
                    if (rr0 + i + 1 < nr) { t += S; st += 2; }
                }
                uint64_t e0 = e00 + (uint64_t)rr0 * p.row_w;
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {
                    const uint32_t a = (src_f + static_cast<uint32_t>(e0)) & 3u;
                    const int c0 = static_cast<int>(4 * q) - static_cast<int>(a);       // column of the granule's first float
                    float o[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float nv = (o[e] - mean[i]) * rsd[i];
                        o[e] = (c0 + e >= 0 && static_cast<uint32_t>(c0 + e) < valid) ? nv : 0.0f;
                    }
                    if (rr0 + i < nr && 4 * q < a + row_w) blm_store4<Out>(dst + e0 + c0, c0, row_w, o);
                    if (rr0 + i + 1 < nr) e0 += p.row_w;
                }
            }
        }
        __syncthreads();
        row0 += nr;
    }
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
constexpr int kBlmNormIoInfo = 6;       // words per staged row: first source float (lo, hi), valid frames, row width, first destination element (lo, hi)

// KEEP IN STEP with blm_normalize_ragged_kernel (fbank512_kernels.hpp; host: blm_norm_shape_ragged), as blm_normalize_io_kernel with its original
template <class Out>
__global__ __launch_bounds__(kBlmNormThreads) MS_NORM_OCCUPANCY void blm_normalize_ragged_io_kernel(const BlmNormRaggedIoParams p) {
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const uint64_t rows = (uint64_t)p.n_clips * p.n_mels;
    const int tid = threadIdx.x;
    const int R = p.rows_per_group, S = p.lds_stride;
    Out *const dst = static_cast<Out *>(p.dst);
    float *stat = tile + (size_t)R * S;      // [R][2]
    float *part = stat + 2 * R;              // [R][PP]
    uint32_t *info = reinterpret_cast<uint32_t *>(part + kBlmNormThreads);     // [R][kBlmNormIoInfo]
    uint32_t *next = info + kBlmNormIoInfo * R;
    const int PP = kBlmNormThreads / R;
    constexpr int kRowsAtOnce = 9;
    const uint32_t src_f = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(p.src) >> 2) & 3u;
    const f4 *src_base = reinterpret_cast<const f4 *>(p.src - src_f);        // the 16-byte granule `src` starts in
    for (;;) {
        if (tid == 0) next[0] = atomicAdd(p.ctr, 1u);
        __syncthreads();
        const uint64_t row0 = (uint64_t)next[0] * R;
        if (row0 >= rows) break;
        const int nr = rows - row0 < (uint64_t)R ? (int)(rows - row0) : R;
        if (tid < nr) {
            const uint64_t row = row0 + tid, clip = row / p.n_mels, m = row - clip * p.n_mels;
            const uint64_t cols = p.d_cols[clip], e0 = p.d_src_off[clip] + m * cols, d0 = p.d_dst_off[clip] + m * cols;
            uint32_t *mine = info + kBlmNormIoInfo * tid;
            mine[0] = static_cast<uint32_t>(e0);
            mine[1] = static_cast<uint32_t>(e0 >> 32);
            mine[2] = static_cast<uint32_t>(p.d_valid[clip]);
            mine[3] = static_cast<uint32_t>(cols);
            mine[4] = static_cast<uint32_t>(d0);
            mine[5] = static_cast<uint32_t>(d0 >> 32);
        }
        __syncthreads();
        uint32_t gmax = 0, wmax = 0;
        for (int rr = 0; rr < nr; ++rr) {
            gmax = info[kBlmNormIoInfo * rr + 2] > gmax ? info[kBlmNormIoInfo * rr + 2] : gmax;
            wmax = info[kBlmNormIoInfo * rr + 3] > wmax ? info[kBlmNormIoInfo * rr + 3] : wmax;
        }
        const uint32_t nq_grp = gmax ? (gmax + 6) / 4 : 0;
        const uint32_t nq_store = wmax ? (wmax + 6) / 4 : 0;
        for (int rr0 = 0; rr0 < nr; rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_grp; q += kBlmNormThreads) {
                f4 v[kRowsAtOnce];
                uint32_t to[kRowsAtOnce];
                uint64_t from[kRowsAtOnce];          // float index of the granule (from the 16-byte aligned base of `src`)
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {
                    const int rr = rr0 + i < nr ? rr0 + i : nr - 1;
                    const uint32_t *ri = info + kBlmNormIoInfo * rr;
                    const uint64_t e0 = ((uint64_t)ri[1] << 32) | ri[0];
                    const uint32_t valid = ri[2];
                    const uint32_t a = (src_f + static_cast<uint32_t>(e0)) & 3u;
                    const uint32_t nq = (a + valid + 3) >> 2;
                    const uint32_t qq = q < nq ? q : (nq ? nq - 1 : 0);
                    from[i] = valid ? src_f + e0 - a + 4 * qq : 0;       // a row without frames owns no memory: the first granule instead
                    to[i] = static_cast<uint32_t>(rr) * S + 4 * qq;
                }
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) v[i] = src_base[from[i] >> 2];
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) *reinterpret_cast<f4 *>(tile + to[i]) = v[i];
            }
        }
        __syncthreads();
        if (tid < nr) {
            const uint32_t valid = info[kBlmNormIoInfo * tid + 2];
            const uint32_t a = (src_f + info[kBlmNormIoInfo * tid]) & 3u;
            MS_PRIO(3);
            stat[2 * tid] = valid ? blm_row_mean_lds(tile + (size_t)tid * S, a, valid) : 0.0f;
            MS_PRIO(0);
        }
        __syncthreads();
        {
            const int r = tid / PP, pt = tid - r * PP;
            if (r < nr) {
                const uint32_t valid = info[kBlmNormIoInfo * r + 2];
                const uint32_t a = (src_f + info[kBlmNormIoInfo * r]) & 3u;
                const float *row = tile + (size_t)r * S + a;
                const float mean = stat[2 * r];
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                uint32_t k = pt;
                for (; k + 3 * PP < valid; k += 4 * PP) {
                    const float c0 = row[k] - mean, c1 = row[k + PP] - mean, c2 = row[k + 2 * PP] - mean, c3 = row[k + 3 * PP] - mean;
                    a0 += c0 * c0; a1 += c1 * c1; a2 += c2 * c2; a3 += c3 * c3;
                }
                for (; k < valid; k += PP) {
                    const float c = row[k] - mean;
                    a0 += c * c;
                }
                part[r * PP + pt] = (a0 + a1) + (a2 + a3);
            }
        }
        __syncthreads();
        if (tid < nr) {
            const float *pp = part + tid * PP;
            float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
            int i = 0;
            for (; i + 3 < PP; i += 4) { q0 += pp[i]; q1 += pp[i + 1]; q2 += pp[i + 2]; q3 += pp[i + 3]; }
            for (; i < PP; ++i) q0 += pp[i];
            float denom = static_cast<float>(info[kBlmNormIoInfo * tid + 2]) - 1.0f;
            denom = denom < 1.0f ? 1.0f : denom;
            const float sd = __builtin_sqrtf(f32_div_rn((q0 + q1) + (q2 + q3), denom)) + 1e-5f;
            stat[2 * tid + 1] = f32_div_rn(1.0f, sd);
        }
        __syncthreads();
        for (int rr0 = 0; rr0 < nr; rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_store; q += kBlmNormThreads) {
                const uint32_t ql = q < nq_grp ? q : nq_grp - 1;      // (nq_store > 0 means a row with frames: nq_grp > 0)
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {
                    const int rr = rr0 + i < nr ? rr0 + i : nr - 1;
                    const uint32_t *ri = info + kBlmNormIoInfo * rr;
                    const uint64_t d0 = ((uint64_t)ri[5] << 32) | ri[4];
                    const uint32_t valid = ri[2], row_w = ri[3];
                    const uint32_t a = (src_f + ri[0]) & 3u;
                    const bool mine = rr0 + i < nr && 4 * q < a + row_w;
                    const f4 v = *reinterpret_cast<const f4 *>(tile + static_cast<uint32_t>(rr) * S + 4 * ql);
                    const float mean = stat[2 * rr], rsd = stat[2 * rr + 1];
                    const int c0 = static_cast<int>(4 * q) - static_cast<int>(a);
                    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float nv = (o[e] - mean) * rsd;
                        o[e] = (c0 + e >= 0 && static_cast<uint32_t>(c0 + e) < valid) ? nv : 0.0f;
                    }
                    if (mine) blm_store4<Out>(dst + d0 + c0, c0, row_w, o);
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace melspec
