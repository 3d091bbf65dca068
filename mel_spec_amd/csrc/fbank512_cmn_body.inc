// fbank512_cmn_body.inc -- the body of the Kaldi fbank's CMN pass, included once per kernel that has it:
//   cmn_kernel<NT> (fbank512_kernels.hpp): in place on the caller's f32 rows, or -- d_means -- the clips' column means alone (the split output);
//   cmn_io_kernel<Out> (fbank512_kaldi_io_kernels.hpp): a 16-bit row cannot have its mean subtracted in place, so the f32 rows are read from a
//     scratch of the object, packed in clip order, and row - mean, rounded once, goes to the caller's rows.
// Staging, the fold of the chunks, the tree (CmnTree) and both forms (staged, column) are this one text, and the host sizes both kernels with
// cmn_shape: the means of a 16-bit call are the f32 call's bits (tests/test_fbank_io_dtypes.py).  Text and not a function for
// fbank512_norm_body.inc's reason.  The _io calls take the 80-bin bank alone, which is always staged: they never run the column form.
// The including kernel has the parameters `p` (b: the clip geometry and the f32 rows, n_mels, rows_per_chunk) and defines
//   NT                    threads of a workgroup
//   Out, kSplit           the row type written; false: in place (the rows of p.b.out), true: p.b.out -> dst
//   dst, d_dst_off        split: the caller's rows and, for ragged batches, the first element of every clip in them (uniform: clip * p.b.out_stride)
//   d_means               not nullptr: write the clip's column means there and no rows (f32 kernel only; nullptr elsewhere: it folds away)
    extern __shared__ __attribute__((aligned(16))) float cmn_lds[];
    const int nm = p.n_mels;
    const int tid = threadIdx.x;
    const int R = p.rows_per_chunk;
    const int nmp = (nm + 3) & ~3;
    float *mean_s = cmn_lds;                 // [nmp]
    float *part_s = cmn_lds + nmp;           // the eight run sums of every column: [8][nmp] (staged form) / [8][NT]
    float *rows = part_s + 8 * (R > 0 ? nmp : NT);
    for (uint32_t clip = blockIdx.x; clip < p.b.n_clips; clip += gridDim.x) {
        const float *o;                 // the clip's f32 rows ...
        Out *d;                         // ... and where they go
        uint64_t frames;
        if (p.b.d_unit_prefix == nullptr) {
            o = p.b.out + (uint64_t)clip * p.b.out_stride;
            if constexpr (kSplit) d = dst + (uint64_t)clip * p.b.out_stride;
            frames = p.b.frames_per_clip;
        } else {
            o = p.b.out + p.b.d_out_off[clip];
            if constexpr (kSplit) d = dst + d_dst_off[clip];
            frames = p.b.d_frames[clip];
        }
        if constexpr (!kSplit) d = const_cast<float *>(o);        // in place
        if (frames == 0) continue;
        if (R > 0) {
            CmnTree tree(frames, part_s + tid, nmp);
            uint64_t f0 = 0;
            const bool vec = ((reinterpret_cast<uintptr_t>(o) & 15) == 0) && (nm % 4 == 0);
            for (;; f0 += R) {
                const int nr = frames - f0 < (uint64_t)R ? (int)(frames - f0) : R;
                const float *src = o + f0 * nm;
                const int total = nr * nm;
                __syncthreads();                                   // the previous chunk has been folded
                if (vec) {
                    // eight 16-byte loads per thread in flight (a plain copy loop leaves one: ~40 memory round trips per chunk)
                    constexpr int kU = 8;
                    const int nq = total / 4;
                    for (int q0 = tid; q0 < nq; q0 += NT * kU) {
                        f4 v[kU];
#pragma unroll
                        for (int k = 0; k < kU; ++k) {
                            const int q = q0 + k * NT;
                            v[k] = *reinterpret_cast<const f4 *>(src + 4 * (q < nq ? q : q0));
                        }
#pragma unroll
                        for (int k = 0; k < kU; ++k) {
                            const int q = q0 + k * NT;
                            if (q < nq) *reinterpret_cast<f4 *>(rows + 4 * q) = v[k];
                        }
                    }
                } else {
                    for (int i = tid; i < total; i += NT) rows[i] = src[i];
                }
                __syncthreads();
                if (tid < nm) {
                    // chunks start at multiples of 4 frames (rows_per_chunk is one): whole units, then the clip's last, partial unit
                    const float *col = rows + tid;
                    const uint64_t ub = f0 / 4;
                    int r = 0;
                    for (; r + 16 <= nr; r += 16) {
                        float v[16];
#pragma unroll
                        for (int i = 0; i < 16; ++i) v[i] = col[(r + i) * nm];
#pragma unroll
                        for (int i = 0; i < 4; ++i) tree.unit(ub + (r >> 2) + i, v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
                    }
                    for (; r + 4 <= nr; r += 4) tree.unit(ub + (r >> 2), col[r * nm], col[(r + 1) * nm], col[(r + 2) * nm], col[(r + 3) * nm]);
                    if (r < nr)
                        tree.unit(ub + (r >> 2), col[r * nm], r + 1 < nr ? col[(r + 1) * nm] : 0.0f, r + 2 < nr ? col[(r + 2) * nm] : 0.0f, 0.0f);
                }
                if (f0 + nr >= frames) break;
            }
            if (tid < nm) mean_s[tid] = f32_div_rn(tree.finish(), (float)frames);
            __syncthreads();
            // the last chunk from LDS, the earlier ones from memory; every row goes to d
            const int nr = (int)(frames - f0);
            const int G = NT / nm;
            const int g = tid / nm, m = tid - g * nm;
            if (d_means) {
                if (tid < nm) d_means[(uint64_t)clip * nm + tid] = mean_s[tid];
            } else if (g < G) {
                const float mean = mean_s[m];
                for (int r = g; r < nr; r += G) d[(f0 + r) * nm + m] = row_value<Out>(rows[r * nm + m] - mean);
                // earlier chunks: 8 rows per thread in flight
                uint64_t f = g;
                for (; f + 7 * (uint64_t)G < f0; f += 8 * (uint64_t)G) {
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = o[(f + k * (uint64_t)G) * nm + m];
#pragma unroll
                    for (int k = 0; k < 8; ++k) d[(f + k * (uint64_t)G) * nm + m] = row_value<Out>(v[k] - mean);
                }
                for (; f < f0; f += G) d[f * nm + m] = row_value<Out>(o[f * nm + m] - mean);
            }
            __syncthreads();                                       // mean_s / rows are reused by the next clip
            continue;
        }
        for (int m0 = 0; m0 < nm; m0 += NT) {                 // column chunks when n_mels > NT
            const int cols = nm - m0 < NT ? nm - m0 : NT;
            const int G = NT / cols;                           // frame groups per column
            const int g = tid / cols, m = m0 + tid - g * cols;
            if (tid < cols) {
                constexpr int kB = 16;
                const float *col = o + m0 + tid;
                CmnTree tree(frames, part_s + tid, NT);
                uint64_t f = 0;
                for (; f + kB <= frames; f += kB) {
                    float v[kB];
#pragma unroll
                    for (int i = 0; i < kB; ++i) v[i] = col[(f + i) * nm];
#pragma unroll
                    for (int i = 0; i < kB / 4; ++i) tree.unit(f / 4 + i, v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
                }
                for (; f + 4 <= frames; f += 4) tree.unit(f / 4, col[f * nm], col[(f + 1) * nm], col[(f + 2) * nm], col[(f + 3) * nm]);
                if (f < frames)
                    tree.unit(f / 4, col[f * nm], f + 1 < frames ? col[(f + 1) * nm] : 0.0f, f + 2 < frames ? col[(f + 2) * nm] : 0.0f, 0.0f);
                rows[tid] = f32_div_rn(tree.finish(), (float)frames);
            }
            __syncthreads();
            if (d_means) {
                if (tid < cols) d_means[(uint64_t)clip * nm + m0 + tid] = rows[tid];
            } else if (g < G) {
                const float mean = rows[tid - g * cols];
                for (uint64_t f = g; f < frames; f += G) d[f * nm + m] = row_value<Out>(o[f * nm + m] - mean);
            }
            __syncthreads();
        }
    }
