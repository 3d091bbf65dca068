// fbank512_kaldi_io_kernels.hpp -- the Kaldi fbank with the sample type (float, int16_t) and the row type (float, f16, bf16) as template
// parameters: melspec_fbank_compute_*_device_io / melspec_fbank_compute_host_io.
//   fbank512_kaldi_io_kernel: the body of fbank512_wave_kernel's Kaldi flavour in its run-per-wave form (the same text, included again):
//     same grid, same runs, same arithmetic; only the loads of fb_kaldi_input (one 4-byte load per int16 sample pair and a 2-byte load for
//     the sample in front of it, times 2^-15, exact; the sample indices of the f32 kernel) and the store of fb_phase3_store (one 16-bit
//     store per lane and value, the f32 value rounded to nearest even once by the store's conversion) differ.  Like its original it has no
//     wait of one wave on another: no barrier in the unit loop, no counter, no polling.
//   cmn_io_kernel: the CMN with a 16-bit output.  A 16-bit row cannot be normalised in place: the main kernel writes its f32 rows, packed in
//     clip order, into a scratch of the object and this pass reads them there -- staging and summation tree exactly those of cmn_kernel --
//     and writes row - mean, rounded once, to the caller's rows: 4 + 2 bytes per element instead of 4 + 4.
// Instantiated in a translation unit of their own (fbank512_kaldi_io.hip): a new neighbour in a unit changes the schedule of the kernels
// that are already there.  fbank512_clip_kernel (the workgroup-per-clip form, whose waves wait for each other) has no such variant.
#pragma once
#include "fbank512_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

template <class T, int WAVES, int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(WAVES * 64, 1) void fbank512_kaldi_io_kernel(const FbankFastParams p) {
    constexpr int FLAVOR = kFlavorKaldi;
    constexpr bool RUNS = true;        // what launch_fused512 runs for this flavour at eight waves (frame-major plain output)
#define MS_FB512_IN In
#define MS_FB512_OUT Out
#include "fbank512_wave_body.inc"
#undef MS_FB512_OUT
#undef MS_FB512_IN
}

struct CmnIoParams {
    BatchDesc b;                // the clip geometry; b.out: the f32 rows, packed in clip order (uniform: b.out_stride apart, ragged: at b.d_out_off)
    void *dst;                  // the caller's rows of the kernel's row type
    const uint64_t *d_dst_off;  // ragged batches: the first element of clip c in dst (uniform batches: c * b.out_stride)
    int n_mels;
    int rows_per_chunk;
};
constexpr int kCmnThreads = 512;      // cmn_kernel<512>'s

// KEEP IN STEP with cmn_kernel (fbank512_kernels.hpp): the staging, the fold of the chunks and the tree (CmnTree) are copies of that
// kernel's, operation for operation, and the host sizes both with cmn_shape (fbank512.hip) -- the means of a 16-bit call are the f32
// call's bits only as long as the two agree.  Only the source / destination split and the final store differ (and the split output's
// d_means, which this pass does not have).
template <class Out>
__global__ __launch_bounds__(kCmnThreads) void cmn_io_kernel(const CmnIoParams p) {
    constexpr int NT = kCmnThreads;
    extern __shared__ __attribute__((aligned(16))) float cmn_lds[];
    const int nm = p.n_mels;
    const int tid = threadIdx.x;
    const int R = p.rows_per_chunk;
    const int nmp = (nm + 3) & ~3;
    float *mean_s = cmn_lds;                 // [nmp]
    float *part_s = cmn_lds + nmp;           // the eight run sums of every column: [8][nmp] (staged form) / [8][NT]
    float *rows = part_s + 8 * (R > 0 ? nmp : NT);
    for (uint32_t clip = blockIdx.x; clip < p.b.n_clips; clip += gridDim.x) {
        const float *o;
        Out *d;
        uint64_t frames;
        if (p.b.d_unit_prefix == nullptr) {
            o = p.b.out + (uint64_t)clip * p.b.out_stride;
            d = static_cast<Out *>(p.dst) + (uint64_t)clip * p.b.out_stride;
            frames = p.b.frames_per_clip;
        } else {
            o = p.b.out + p.b.d_out_off[clip];
            d = static_cast<Out *>(p.dst) + p.d_dst_off[clip];
            frames = p.b.d_frames[clip];
        }
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
            // the last chunk from LDS, the earlier ones from the scratch; every row goes to the caller
            const int nr = (int)(frames - f0);
            const int G = NT / nm;
            const int g = tid / nm, m = tid - g * nm;
            if (g < G) {
                const float mean = mean_s[m];
                for (int r = g; r < nr; r += G) d[(f0 + r) * nm + m] = row_value<Out>(rows[r * nm + m] - mean);
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
        // the column form (banks wider than the staging allows: cmn_shape picks it for more than 512 bins only, whatever the clips'
        // length): folded from the scratch.  NOT RUN today -- the _io calls take the 80-bin bank alone, which is always staged -- and so
        // not tested; carried only so that this kernel mirrors cmn_kernel form for form and a wider bank needs no new kernel.
        for (int m0 = 0; m0 < nm; m0 += NT) {
            const int cols = nm - m0 < NT ? nm - m0 : NT;
            const int G = NT / cols;
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
            if (g < G) {
                const float mean = rows[tid - g * cols];
                for (uint64_t f = g; f < frames; f += G) d[f * nm + m] = row_value<Out>(o[f * nm + m] - mean);
            }
            __syncthreads();
        }
    }
}

}  // namespace melspec
