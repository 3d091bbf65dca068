// fbank512_norm_ragged_body.inc -- the body of the NeMo frontend's per-feature normaliser over a ragged batch, included once per kernel that
// has it: blm_normalize_ragged_kernel (fbank512_kernels.hpp, in place on f32 rows) and blm_normalize_ragged_io_kernel<Out>
// (fbank512_io_kernels.hpp, f32 rows of a scratch -> the caller's 16-bit rows, pad columns included); fbank512_norm_body.inc says why it
// is one text and why text.  The host sizes both kernels with blm_norm_shape_ragged.
// The including kernel has the parameters `p` (n_clips, n_mels, rows_per_group, lds_stride, d_cols, d_valid, ctr) and defines
//   Out, kSplit           the row type written; false: in place, true: src -> dst
//   src, dst              the f32 rows read and the rows written (in place: the same)
//   d_src_off, d_dst_off  per clip the first element in src / dst
// and may define MS_NORM_RAGGED_ORDER (blm_normalize_ragged_desc_kernel): the number of threads, at most PP, that share a row's sum of squares
// -- the order of that sum -- where it is not the launch's own PP; without the macro the text below is what it always was.
#ifndef MS_NORM_RAGGED_ORDER
#define MS_NORM_RAGGED_ORDER PP
#define MS_NORM_RAGGED_IN_ORDER(pt) true
#define MS_NORM_RAGGED_ORDER_DEFAULT
#else
#define MS_NORM_RAGGED_IN_ORDER(pt) ((pt) < MS_NORM_RAGGED_ORDER)
#endif
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const uint64_t rows = (uint64_t)p.n_clips * p.n_mels;
    const int tid = threadIdx.x;
    const int R = p.rows_per_group, S = p.lds_stride;
    float *stat = tile + (size_t)R * S;      // [R][2]
    float *part = stat + 2 * R;              // [R][PP]
    constexpr int kInfo = kSplit ? kBlmNormIoInfo : kBlmNormInfo;
    uint32_t *info = reinterpret_cast<uint32_t *>(part + kBlmNormThreads);     // [R][kInfo]: first float in src (lo, hi), valid frames, row width [, first element in dst (lo, hi)]
    uint32_t *next = info + kInfo * R;
    const int PP = kBlmNormThreads / R;
    constexpr int kRowsAtOnce = 9;
    const uint32_t src_f = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) >> 2) & 3u;
    const f4 *src_base = reinterpret_cast<const f4 *>(src - src_f);        // the 16-byte granule `out` starts in
    for (;;) {
        if (tid == 0) next[0] = atomicAdd(p.ctr, 1u);
        __syncthreads();
        const uint64_t row0 = (uint64_t)next[0] * R;
        if (row0 >= rows) break;
        const int nr = rows - row0 < (uint64_t)R ? (int)(rows - row0) : R;
        if (tid < nr) {
            const uint64_t row = row0 + tid, clip = row / p.n_mels, m = row - clip * p.n_mels;
            const uint64_t cols = p.d_cols[clip], e0 = d_src_off[clip] + m * cols;
            info[kInfo * tid] = static_cast<uint32_t>(e0);
            info[kInfo * tid + 1] = static_cast<uint32_t>(e0 >> 32);
            info[kInfo * tid + 2] = static_cast<uint32_t>(p.d_valid[clip]);
            info[kInfo * tid + 3] = static_cast<uint32_t>(cols);
            if constexpr (kSplit) {
                const uint64_t d0 = d_dst_off[clip] + m * cols;
                info[kInfo * tid + 4] = static_cast<uint32_t>(d0);
                info[kInfo * tid + 5] = static_cast<uint32_t>(d0 >> 32);
            }
        }
        __syncthreads();
        // granules of the longest row OF THIS GROUP (round 5: both copy loops ran to the longest row of the batch -- clips of 5..15 s
        // made a third of their iterations re-read and re-write a short row's last granule)
        uint32_t gmax = 0, wmax = 0;
        for (int rr = 0; rr < nr; ++rr) {
            gmax = info[kInfo * rr + 2] > gmax ? info[kInfo * rr + 2] : gmax;
            if constexpr (kSplit) wmax = info[kInfo * rr + 3] > wmax ? info[kInfo * rr + 3] : wmax;
        }
        const uint32_t nq_grp = gmax ? (gmax + 6) / 4 : 0;
        // in place: the granules that hold valid frames; split: every granule of the row (normalised values, then zeros up to row_w)
        const uint32_t nq_store = kSplit ? (wmax ? (wmax + 6) / 4 : 0) : nq_grp;
        for (int rr0 = 0; rr0 < nr; rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_grp; q += kBlmNormThreads) {
                f4 v[kRowsAtOnce];
                uint32_t to[kRowsAtOnce];
                uint64_t from[kRowsAtOnce];          // float index of the granule (from the 16-byte aligned base of `src`)
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {
                    const int rr = rr0 + i < nr ? rr0 + i : nr - 1;
                    const uint64_t e0 = ((uint64_t)info[kInfo * rr + 1] << 32) | info[kInfo * rr];
                    const uint32_t valid = info[kInfo * rr + 2];
                    const uint32_t a = (src_f + static_cast<uint32_t>(e0)) & 3u;
                    const uint32_t nq = (a + valid + 3) >> 2;
                    const uint32_t qq = q < nq ? q : (nq ? nq - 1 : 0);
                    from[i] = valid ? src_f + e0 - a + 4 * qq : 0;       // a row without frames may own no memory at all: the first granule instead
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
            const uint32_t valid = info[kInfo * tid + 2];
            const uint32_t a = (src_f + info[kInfo * tid]) & 3u;
            MS_PRIO(3);
            stat[2 * tid] = valid ? blm_row_mean_lds(tile + (size_t)tid * S, a, valid) : 0.0f;
            MS_PRIO(0);
        }
        __syncthreads();
        {
            const int r = tid / PP, pt = tid - r * PP;
            if (r < nr && MS_NORM_RAGGED_IN_ORDER(pt)) {
                const uint32_t valid = info[kInfo * r + 2];
                const uint32_t a = (src_f + info[kInfo * r]) & 3u;
                const float *row = tile + (size_t)r * S + a;
                const float mean = stat[2 * r];
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f;
                uint32_t k = pt;
                for (; k + 3 * MS_NORM_RAGGED_ORDER < valid; k += 4 * MS_NORM_RAGGED_ORDER) {
                    const float c0 = row[k] - mean, c1 = row[k + MS_NORM_RAGGED_ORDER] - mean, c2 = row[k + 2 * MS_NORM_RAGGED_ORDER] - mean, c3 = row[k + 3 * MS_NORM_RAGGED_ORDER] - mean;
                    a0 += c0 * c0; a1 += c1 * c1; a2 += c2 * c2; a3 += c3 * c3;
                }
                for (; k < valid; k += MS_NORM_RAGGED_ORDER) {
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
            for (; i + 3 < MS_NORM_RAGGED_ORDER; i += 4) { q0 += pp[i]; q1 += pp[i + 1]; q2 += pp[i + 2]; q3 += pp[i + 3]; }
            for (; i < MS_NORM_RAGGED_ORDER; ++i) q0 += pp[i];
            float denom = static_cast<float>(info[kInfo * tid + 2]) - 1.0f;
            denom = denom < 1.0f ? 1.0f : denom;
            const float sd = __builtin_sqrtf(f32_div_rn((q0 + q1) + (q2 + q3), denom)) + 1e-5f;
            stat[2 * tid + 1] = f32_div_rn(1.0f, sd);
        }
        __syncthreads();
        for (int rr0 = 0; rr0 < nr; rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_store; q += kBlmNormThreads) {
                const uint32_t ql = kSplit && q >= nq_grp ? nq_grp - 1 : q;      // granules past the staged frames: the last staged one, never used (nq_store > 0 means a row with frames: nq_grp > 0)
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) {
                    const int rr = rr0 + i < nr ? rr0 + i : nr - 1;
                    const uint64_t e0 = ((uint64_t)info[kInfo * rr + 1] << 32) | info[kInfo * rr];
                    const uint64_t d0 = kSplit ? ((uint64_t)info[kInfo * rr + kInfo - 1] << 32) | info[kInfo * rr + kInfo - 2] : e0;
                    const uint32_t valid = info[kInfo * rr + 2], row_w = info[kInfo * rr + 3];
                    const uint32_t a = (src_f + static_cast<uint32_t>(e0)) & 3u;
                    const bool mine = rr0 + i < nr && (kSplit ? 4 * q < a + row_w : valid != 0 && 4 * q < a + valid);
                    const f4 v = *reinterpret_cast<const f4 *>(tile + static_cast<uint32_t>(rr) * S + 4 * ql);
                    const float mean = stat[2 * rr], rsd = stat[2 * rr + 1];
                    const int c0 = static_cast<int>(4 * q) - static_cast<int>(a);
                    float o[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float nv = (o[e] - mean) * rsd;
                        o[e] = (c0 + e >= 0 && static_cast<uint32_t>(c0 + e) < valid) ? nv : 0.0f;
                    }
                    Out *g = dst + d0 + c0;
                    if (mine) {
                        if constexpr (kSplit) {
                            blm_store4(g, c0, row_w, o);
                        } else if (c0 >= 0 && static_cast<uint32_t>(c0 + 3) < row_w) {
                            f4 w = {o[0], o[1], o[2], o[3]};
                            *reinterpret_cast<f4 *>(g) = w;
                        } else {
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (c0 + e >= 0 && static_cast<uint32_t>(c0 + e) < row_w) g[e] = o[e];
                        }
                    }
                }
            }
        }
        __syncthreads();
    }
#ifdef MS_NORM_RAGGED_ORDER_DEFAULT
#undef MS_NORM_RAGGED_ORDER
#undef MS_NORM_RAGGED_ORDER_DEFAULT
#endif
#undef MS_NORM_RAGGED_IN_ORDER
