// fbank512_norm_body.inc -- the body of the NeMo frontend's per-feature normaliser over a uniform batch, included once per kernel that has it:
//   blm_normalize_kernel (fbank512_kernels.hpp): in place on the caller's f32 rows -- the store phase reaches the valid frames only (the pad
//     columns keep the zeros the mel kernel wrote);
//   blm_normalize_io_kernel<Out> (fbank512_io_kernels.hpp): a 16-bit row cannot be normalised in place, so the f32 rows are read from a scratch
//     of the context and every column of the row goes to the caller's rows -- (v - mean) / sd rounded once, then the zero pad columns up to row_w.
// Staging, mean fold, sum-of-squares tree and sd are this one text, and the host sizes both kernels with blm_norm_shape_uniform: the
// statistics of a 16-bit call are the f32 call's bits (tests/test_blm_io_dtypes.py).  It is text and not a function because the f32 kernel's
// instructions were not to change: behind an inlined function -- the kernel's own statements, untouched -- its schedule comes out different.
// The including kernel has the parameters `p` (n_clips, n_mels, rows_per_group, lds_stride, row_w, valid, d_cols, d_valid) and defines
//   Out, kSplit           the row type written; false: in place, true: src -> dst
//   src, dst              the f32 rows read and the rows written (in place: the same)
//   d_src_off, d_dst_off  ragged batches (rows_per_group == 0 form only): per clip the first element in src / dst
//   clip_stride           elements between clips
//   fold_sel, lab_skip, dbg   the lab switches of the f32 kernel (-1, 0, nullptr elsewhere: they fold away)
    extern __shared__ __attribute__((aligned(16))) float tile[];
    const uint64_t rows = (uint64_t)p.n_clips * p.n_mels;
    const int tid = threadIdx.x;
    (void)dbg;
    if (p.rows_per_group == 0) {
        for (uint64_t row = (uint64_t)blockIdx.x * kBlmNormThreads + tid; row < rows; row += (uint64_t)gridDim.x * kBlmNormThreads) {
            const float *r;
            Out *d;
            uint64_t valid = p.valid, cols = p.row_w;
            if (d_dst_off) {
                const uint64_t clip = row / p.n_mels, m = row - clip * p.n_mels;
                r = src + d_src_off[clip] + m * p.d_cols[clip];
                if constexpr (kSplit) {
                    cols = p.d_cols[clip];
                    d = dst + d_dst_off[clip] + m * cols;
                }
                valid = p.d_valid[clip];
                if (valid == 0) {
                    if constexpr (kSplit)
                        for (uint64_t k = 0; k < cols; ++k) d[k] = static_cast<Out>(0.0f);
                    continue;
                }
            } else {
                const uint64_t clip = row / p.n_mels, m = row - clip * p.n_mels;
                r = src + clip * clip_stride + m * p.row_w;
                if constexpr (kSplit) d = dst + clip * clip_stride + m * p.row_w;
            }
            if constexpr (!kSplit) d = const_cast<float *>(r);        // in place
            float mean, sd;
            blm_row_stats_slow(r, valid, mean, sd);
            for (uint64_t k = 0; k < valid; ++k) d[k] = row_value<Out>(f32_div_rn(r[k] - mean, sd));
            if constexpr (kSplit)
                for (uint64_t k = valid; k < cols; ++k) d[k] = static_cast<Out>(0.0f);
        }
        return;
    }
    const int R = p.rows_per_group, S = p.lds_stride;
    float *stat = tile + (size_t)R * S;      // [R][2]
    const int fold_wave = fold_sel < 0 ? 0 : static_cast<int>((blockIdx.x >> (fold_sel < 0 ? 0 : fold_sel)) & 3u);
    // Rows of one clip are contiguous and so are the clips (clip_stride == n_mels * row_w): row r starts at src + r * row_w, at
    // any 4-byte alignment (1001 columns for a 10 s clip without pad_to).  Global memory is read in whole 16-byte granules
    // all the same: a row whose first float sits `a` floats into its granule is staged from the granule's start, at the same
    // offset `a` in its 16-byte aligned LDS row; in place, the granules a row shares with its neighbours are loaded by both and stored
    // float by float.  kRowsAtOnce rows in flight per thread (a load inside a per-row `if` would be one memory round trip per
    // row; rows past the group re-read its last row, granules past the row its last granule).
    constexpr int kRowsAtOnce = 9;
    const uint32_t valid = static_cast<uint32_t>(p.valid);
    const uint32_t src_f = static_cast<uint32_t>(reinterpret_cast<uintptr_t>(src) >> 2) & 3u;
    const uint32_t nq_max = (valid + 6) / 4;            // granules of a row's valid frames at the worst alignment
    // A workgroup owns a contiguous range of rows and walks it in rounds of R.  (Starting the workgroups out of step -- a short
    // first round, a sleep per workgroup -- was measured: no effect; once its phases are cheap the pass is bandwidth-bound.)
    const uint64_t per_wg = (rows + gridDim.x - 1) / gridDim.x;
    const uint64_t row_begin = (uint64_t)blockIdx.x * per_wg;
    const uint64_t row_end = row_begin + per_wg < rows ? row_begin + per_wg : rows;
    float *part = stat + 2 * R;              // [R][PP] partial sums of squares
    uint64_t stamp = 0;
    (void)stamp;
    const int PP = kBlmNormThreads / R;      // threads per row in the variance pass
    for (uint64_t row0 = row_begin; row0 < row_end;) {
        MS_NORM_STAMP(0);
        const int nr = row_end - row0 < (uint64_t)R ? (int)(row_end - row0) : R;
        const uint64_t e00 = row0 * p.row_w;
        for (int rr0 = 0; rr0 < ((lab_skip & 4) ? 0 : nr); rr0 += kRowsAtOnce) {
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
                    v[i] = *reinterpret_cast<const f4 *>(src + e0 - a + 4 * qq);
                    to[i] = t + 4 * qq;
                    if (rr0 + i + 1 < nr) { e0 += p.row_w; t += S; }
                }
#pragma unroll
                for (int i = 0; i < kRowsAtOnce; ++i) *reinterpret_cast<f4 *>(tile + to[i]) = v[i];
            }
        }
        __syncthreads();
        MS_NORM_STAMP(1);
        // the means: a few lanes of ONE wave (fold_sel: which one; measured without effect)
        const int ft = tid - 64 * fold_wave;
        if (ft >= 0 && ft < nr) {
            const uint32_t a = (src_f + static_cast<uint32_t>(e00 + (uint64_t)ft * p.row_w)) & 3u;
            MS_PRIO(3);                          // a chain of dependent adds: every issue slot it is ready for
            stat[2 * ft] = (lab_skip & 1) ? 0.0f : blm_row_mean_lds(tile + (size_t)ft * S, a, valid);
            MS_PRIO(0);
        }
        __syncthreads();
        MS_NORM_STAMP(2);
        // the unbiased variance: sum of (v - mean)^2 as a fixed tree over all threads, PP strided partial sums per row added in
        // order.  The reference folds this sum left to right as well; unlike the mean, the order is immaterial here -- either
        // sum is within ~1e-6 (relative) of the exact one, 5e-7 of the standard deviation, and the output moves by |out| * 5e-7.
        {
            const int r = tid / PP, pt = tid - r * PP;
            if (r < nr) {
                const uint32_t a = (src_f + static_cast<uint32_t>(e00 + (uint64_t)r * p.row_w)) & 3u;
                const float *row = tile + (size_t)r * S + a;
                const float mean = stat[2 * r];
                // four sums in turn: the strided loop has a run-time step, and with one accumulator every LDS read waited for
                // the add before it (2.1 us per round, measured with MS_NORM_STAMP; 36 values per thread at 1001 frames)
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
        MS_NORM_STAMP(3);
        if (tid < nr) {
            const float *pp = part + tid * PP;
            float q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, q3 = 0.0f;
            int i = 0;
            for (; i + 3 < PP; i += 4) { q0 += pp[i]; q1 += pp[i + 1]; q2 += pp[i + 2]; q3 += pp[i + 3]; }
            for (; i < PP; ++i) q0 += pp[i];
            const float q = (q0 + q1) + (q2 + q3);
            float denom = static_cast<float>(valid) - 1.0f;
            denom = denom < 1.0f ? 1.0f : denom;
            // the row's values are multiplied by 1 / (std + 1e-5) below: within one ulp of the reference's division, 9 divisions
            // per round instead of 36 per thread (the divisions were 4.7 us of a 16 us round)
            const float sd = __builtin_sqrtf(f32_div_rn(q, denom)) + 1e-5f;
            stat[2 * tid + 1] = (lab_skip & 1) ? 1.0f : f32_div_rn(1.0f, sd);
        }
        __syncthreads();
        MS_NORM_STAMP(4);
        const uint32_t row_w = static_cast<uint32_t>(p.row_w);
        // in place: the granules that hold valid frames; split: every granule of the row (normalised values, then zeros up to row_w)
        const uint32_t nq_store = kSplit ? (row_w + 6) / 4 : nq_max;
        for (int rr0 = 0; rr0 < ((lab_skip & 2) ? 0 : nr); rr0 += kRowsAtOnce) {
            for (uint32_t q = tid; q < nq_store; q += kBlmNormThreads) {
                f4 v[kRowsAtOnce];
                float mean[kRowsAtOnce], rsd[kRowsAtOnce];
                const uint32_t ql = kSplit && q >= nq_max ? nq_max - 1 : q;      // granules past the staged frames: the last staged one, never used
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
                    for (int e = 0; e < 4; ++e) {                 // columns past the valid frames are zeros
                        const float nv = (o[e] - mean[i]) * rsd[i];
                        o[e] = (c0 + e >= 0 && static_cast<uint32_t>(c0 + e) < valid) ? nv : 0.0f;
                    }
                    Out *g = dst + e0 + c0;
                    const bool mine = rr0 + i < nr && 4 * q < a + (kSplit ? row_w : valid);     // granules that hold columns to store of a row of the group
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
                    if (rr0 + i + 1 < nr) e0 += p.row_w;
                }
            }
        }
        __syncthreads();
        MS_NORM_STAMP(5);
        row0 += nr;
    }
