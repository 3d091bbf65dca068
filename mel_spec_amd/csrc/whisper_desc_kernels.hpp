// whisper_desc_kernels.hpp -- the kernels of the centred Whisper features on a clip table that lives in device memory
// (melspec_whisper_compute_ragged_device_desc*; whisper_centered.hip launches them, whisper_centered_plan.hpp has the plan buffer's layout
// and the per-thread functions, which tests/cpp/whisper_desc_plan_host.cpp runs on the host):
//   wc_plan_desc_kernel          one workgroup, partials -> scan -> write (plan_ragged_device_kernel's shape): the clips' records, the
//                                interior as a table for plan_ragged_device_kernel, the compacted edge list and the edge launch's batch
//   wc_prepare_desc_kernel<In>   wc_prepare_kernel with the number of edge frames read from the plan: the launch is sized for five per clip,
//                                a block past the true count does nothing
// Kernels of their own beside the existing ones, which keep their code.
#pragma once
#include "whisper_centered_kernels.hpp"

namespace melspec {

struct WcPlanDescParams {
    host::WcDescIn in;
    void *plan;          // host::wc_desc_bytes(n_clips)
};

__global__ __launch_bounds__(1024) void wc_plan_desc_kernel(const WcPlanDescParams q) {
    static_assert(host::kWcDescThreads == 1024 && host::kWcDescUnitBlock == kUnitBlock, "the plan's constants");
    __shared__ uint64_t wave_edges[16];
    const uint32_t tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const host::WcDescTables t = host::wc_desc_tables(q.plan, q.in.n_clips);
    uint32_t c0, c1;
    host::wc_desc_slice(q.in.n_clips, tid, c0, c1);
    const uint64_t mine = host::wc_desc_count(q.in, c0, c1);
    // inclusive sum over the wave's lanes, then sixteen wave totals that every thread adds up for itself (blm_plan_ragged_device_kernel)
    uint64_t incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up(static_cast<unsigned long long>(incl), d);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wave_edges[wave] = incl;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        const uint64_t e = wave_edges[w];
        if (w < wave) before += e;
        all += e;
    }
    if (tid == 0) *t.n_edges = all;
    host::wc_desc_fixed(t, q.in.n_clips, tid);
    host::wc_desc_write(q.in, t, c0, c1, before + incl - mine);
}

// work items [0, 5 n_clips): item e gathers edge frame e if e < *n_edges (host::wc_source_index's rule; no sample at or past n_eff is read);
// the items behind them: 256 maximum words each.  One item per block up to the grid limit, a grid-stride loop past it (the launch takes
// min(items, 2^31 - 1) blocks: 5 n_clips alone reaches 2^32 - 1 at the calls' clip bound)
template <class In>
__global__ __launch_bounds__(256) void wc_prepare_desc_kernel(const In *pcm, const host::WcEdge *edges, const uint64_t *n_edges, uint32_t cap, float *edge_pcm,
                                                              int *slots, uint32_t n_slots) {
    const uint64_t items = static_cast<uint64_t>(cap) + (static_cast<uint64_t>(n_slots) + 255) / 256, true_edges = *n_edges;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        if (item >= cap) {
            const uint64_t i = (item - cap) * 256 + threadIdx.x;
            if (i < n_slots) slots[i] = kWcFloorBits;
            continue;
        }
        if (item >= true_edges) continue;
        const host::WcEdge e = edges[item];
        host::WcClip c{};
        c.n_eff = e.n_eff; c.P = e.P;
        const In *src = pcm + e.pcm_off;
        float *dst = edge_pcm + item * host::kWcFft;
        for (unsigned i = threadIdx.x; i < host::kWcFft; i += 256) {
            const int64_t idx = host::wc_source_index(c, e.t, i);
            dst[i] = idx >= 0 ? pcm_value(src[idx]) : 0.0f;
        }
    }
}

}  // namespace melspec
