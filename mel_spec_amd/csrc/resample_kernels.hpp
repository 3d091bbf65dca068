// resample_kernels.hpp -- the polyphase windowed-sinc resampler's kernel (melspec_resample_*; resample_plan.hpp has the definition, the
// tap table and the tile arithmetic, resample.hip the entry points).
//
// One 256-thread workgroup per tile of consecutive output blocks of one clip, in a grid-stride loop over the call's tiles so that the tap
// table is read into LDS once per workgroup.  The tile's samples, with the filter's halo and zeros outside the clip, are staged in LDS as
// f64 (an int16 sample is s * 2^-15, exactly): 16-byte global loads from the first 16-byte boundary on, single elements in front of it and
// behind the last whole vector.  Consecutive lanes compute consecutive outputs: lane o reads its phase's window tap-major (consecutive
// phases are consecutive words; one phase: a broadcast) and its samples from (o / new) * orig + start[phase] on -- 8-byte reads, whose
// bank is (address / 4) mod 64, so the stride of orig = 3 doubles of 48 kHz -> 16 kHz is conflict-free.  Products and sums are f64 in
// ascending tap order with fused multiply-adds, rounded to f32 once at the store: an output's bits depend on its own window alone, not on
// the tile, the batch or the entry point.
//   kRsLdsAll      samples and taps in LDS (every usual rate)
//   kRsLdsSamples  the tap table does not fit beside the samples: it is read from its global, read-only table
//   kRsGlobal      one block's samples do not fit either (ratios in the thousands): every sample is read from the clip, bounds-checked
//   kRsCopy        rate_in == rate_out: the converted input
#pragma once
#include <hip/hip_runtime.h>

#include "io_types.hpp"
#include "resample_plan.hpp"

namespace melspec {

struct RsKernelGeom {
    uint32_t orig, nw, width, taps, blocks;
};

__device__ __forceinline__ double rs_value(float v) { return static_cast<double>(v); }
__device__ __forceinline__ double rs_value(io_s16 v) { return static_cast<double>(v) * 0x1p-15; }

// the 16 bytes of a vector load as 4 floats / 8 int16 samples, element e
template <class S> struct RsVec;
template <> struct RsVec<float> {
    static constexpr uint32_t kElems = 4;
    static __device__ __forceinline__ void unpack(const uint4 &q, double *dst) {
        dst[0] = rs_value(__uint_as_float(q.x)); dst[1] = rs_value(__uint_as_float(q.y));
        dst[2] = rs_value(__uint_as_float(q.z)); dst[3] = rs_value(__uint_as_float(q.w));
    }
};
template <> struct RsVec<io_s16> {
    static constexpr uint32_t kElems = 8;
    static __device__ __forceinline__ void unpack(const uint4 &q, double *dst) {
        const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dst[2 * i] = rs_value(static_cast<io_s16>(w[i] & 0xffffu));
            dst[2 * i + 1] = rs_value(static_cast<io_s16>(w[i] >> 16));
        }
    }
};

template <class S, int MODE>
__global__ __launch_bounds__(256) void resample_kernel(const S *__restrict__ pcm, float *__restrict__ out, const host::RsClip *__restrict__ tab,
                                                       uint32_t n_clips, uint64_t n_tiles, RsKernelGeom kg, const double *__restrict__ win,
                                                       const uint32_t *__restrict__ start) {
    using namespace host;
    extern __shared__ double rs_lds[];
    const uint32_t tid = threadIdx.x;
    const uint32_t span = MODE <= kRsLdsSamples ? static_cast<uint32_t>(rs_span(kg.orig, kg.width, kg.blocks)) : 0;
    double *xs = rs_lds;
    double *lw = xs + span;
    uint32_t *ls = reinterpret_cast<uint32_t *>(lw + static_cast<size_t>(kg.taps) * kg.nw);
    if (MODE == kRsLdsAll) {      // visible behind the first tile's barriers
        for (uint32_t i = tid; i < kg.taps * kg.nw; i += kRsThreads) lw[i] = win[i];
        for (uint32_t i = tid; i < kg.nw; i += kRsThreads) ls[i] = start[i];
    }
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const RsClip rec = tab[rs_find_clip(tab, n_clips, t)];
        const RsTile tl = rs_tile(kg.orig, kg.nw, MODE == kRsCopy ? 0 : kg.width, kg.blocks, rec.len, t - rec.tile0);
        const S *x = pcm + rec.in_off;
        float *y = out + rec.out_off + tl.o0;
        if (MODE == kRsCopy) {
            for (uint32_t o = tid; o < tl.n_out; o += kRsThreads) y[o] = static_cast<float>(rs_value(x[tl.o0 + o]));
            continue;
        }
        if (MODE <= kRsLdsSamples) {
            __syncthreads();      // the tile before this one has been read
            for (uint32_t i = tid; i < tl.lo; i += kRsThreads) xs[i] = 0.0;
            for (uint32_t i = tl.hi + tid; i < tl.span; i += kRsThreads) xs[i] = 0.0;
            const S *g = x + (tl.s0 + static_cast<int64_t>(tl.lo));      // the first sample inside the clip: s0 + lo >= 0
            const uint32_t n = tl.hi - tl.lo;
            uint32_t head = static_cast<uint32_t>(((16u - (reinterpret_cast<uintptr_t>(g) & 15u)) & 15u) / sizeof(S));
            if (head > n) head = n;
            const uint32_t nv = (n - head) / RsVec<S>::kElems, body = nv * RsVec<S>::kElems;
            double *dst = xs + tl.lo;
            for (uint32_t i = tid; i < head; i += kRsThreads) dst[i] = rs_value(g[i]);
            const uint4 *gv = reinterpret_cast<const uint4 *>(g + head);      // 16-byte aligned by the choice of head
            for (uint32_t v = tid; v < nv; v += kRsThreads) {
                const uint4 q = gv[v];
                RsVec<S>::unpack(q, dst + head + v * RsVec<S>::kElems);
            }
            for (uint32_t i = head + body + tid; i < n; i += kRsThreads) dst[i] = rs_value(g[i]);
            __syncthreads();
        }
        for (uint32_t o = tid; o < tl.n_out; o += kRsThreads) {
            const uint32_t jb = o / kg.nw, p = o - jb * kg.nw;
            const uint32_t base = jb * kg.orig + (MODE == kRsLdsAll ? ls[p] : start[p]);      // + t < blocks * orig + 2 * width
            const double *wp = (MODE == kRsLdsAll ? lw : win) + p;
            double acc = 0.0;
            if (MODE <= kRsLdsSamples) {
                const double *xp = xs + base;
#pragma unroll 4
                for (uint32_t k = 0; k < kg.taps; ++k) acc = fma(wp[static_cast<size_t>(k) * kg.nw], xp[k], acc);
            } else {
                const int64_t s = tl.s0 + static_cast<int64_t>(base), len = static_cast<int64_t>(rec.len);
                for (uint32_t k = 0; k < kg.taps; ++k) {
                    const int64_t i = s + k;
                    const double v = i >= 0 && i < len ? rs_value(x[i]) : 0.0;
                    acc = fma(wp[static_cast<size_t>(k) * kg.nw], v, acc);
                }
            }
            y[o] = static_cast<float>(acc);
        }
    }
}

}  // namespace melspec
