// whisper_centered_plan.hpp -- the host side of the centred Whisper features (melspec_whisper_*, whisper_centered.hip) that is arithmetic
// only: the frame count of a clip, the class of every frame (interior / edge / silent), the interior of a batch as a plain ragged batch for
// the existing planners, the list of edge frames, the per-clip records of the fill / finalise passes, and the checks of the calls'
// arguments in their order; for the calls with int16 PCM in / f16, bf16 out (melspec_whisper_*_io) the element sizes, the alignment rule
// and the 16-byte store rule of the finalise pass; for the calls whose clip table lives in device memory (melspec_whisper_*_desc*) the plan
// buffer's layout and the per-thread functions of the planner kernel.  Nothing from HIP in here but the host-device qualifier:
// tests/cpp/whisper_centered_host.cpp, tests/cpp/whisper_centered_io_host.cpp and tests/cpp/whisper_desc_plan_host.cpp build it on the
// host, with and without sanitizers.
//
// A clip x of n samples under pad_to (0: as it is) is the signal s = x[:pad_to] + zeros up to pad_to, P = len(s) samples, of which the
// first n_eff = min(n, P) are the caller's.  T = P / 160 frames (0 when P < 400); frame t is r[160 t .. 160 t + 400) of
// r = reflect_pad(s, 200), i.e. the samples s[160 t - 200 .. 160 t + 200) with indices < 0 mirrored at 0 and indices >= P mirrored at
// P - 1 (numpy.pad(mode = "reflect"), torch.stft(center = True)).
//   interior  2 <= t and 160 t + 200 <= n_eff: an ordinary un-centred frame, number t - 2, of the clip that starts 120 samples in
//   silent    every sample the frame reads is a zero of the extension: n_eff == 0, or t >= 2 and 160 t - 200 >= n_eff (a mirrored index
//             at the right end is never below the window's first: 2 (P - 1) - (160 t + 199) >= 160 t - 200 for every t < T)
//   edge      the rest: frames 0 and 1 (they mirror at 0) and the frames that straddle n_eff or mirror at P - 1 -- at most three
// The classes are runs: [0, 2) edge (silent when n_eff == 0), [2, 2 + interior) interior, [2 + interior, first_silent) edge,
// [first_silent, T) silent.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/melspec_hip.h"

// the per-clip arithmetic is one text for the host and for the planner / gather kernels of the _desc calls (blm_desc_plan.hpp: MS_BLM_HD)
#if defined(__HIPCC__)
#define MS_WC_HD __host__ __device__ inline
#else
#define MS_WC_HD inline
#endif

namespace melspec {
namespace host {

constexpr uint64_t kWcFft = 400, kWcHop = 160, kWcPad = 200;
constexpr uint64_t kWcShift = 120;          // 2 * hop - pad: where the interior "clip" starts; 480 bytes, a 16-byte aligned start stays one
constexpr uint64_t kWcMaxEdges = 5;         // per clip: frames 0, 1 and at most three at the end of the samples
constexpr float kWcFloorLog = -10.0f;       // log10(1e-10): a silent frame's raw value and the clip maximum of a clip without a frame

enum WcClass { kWcInterior = 0, kWcEdge = 1, kWcSilent = 2 };

struct WcClip {
    uint64_t n_eff;          // samples of the caller's inside the signal
    uint64_t P;              // length of the signal
    uint64_t T;              // frames
    uint64_t interior;       // frames 2 .. 2 + interior - 1
    uint64_t first_silent;   // frames first_silent .. T - 1 (== T: none)
};

MS_WC_HD WcClip wc_clip(uint64_t n, uint64_t pad_to) {
    WcClip c{};
    c.P = pad_to ? pad_to : n;
    c.n_eff = n < c.P ? n : c.P;
    c.T = c.P < kWcFft ? 0 : c.P / kWcHop;
    if (c.T == 0) return c;
    if (c.n_eff == 0) return c;                                   // first_silent = 0: every frame is silent
    const uint64_t t_max = c.n_eff >= kWcPad ? (c.n_eff - kWcPad) / kWcHop : 0;      // last t with 160 t + 200 <= n_eff
    c.interior = t_max >= 2 ? t_max - 1 : 0;
    uint64_t s = (c.n_eff + kWcPad + kWcHop - 1) / kWcHop;        // first t with 160 t - 200 >= n_eff
    if (s < 2) s = 2;
    c.first_silent = s < c.T ? s : c.T;
    return c;
}
inline uint64_t wc_num_frames(uint64_t n, uint64_t pad_to) { return wc_clip(n, pad_to).T; }
MS_WC_HD WcClass wc_class(const WcClip &c, uint64_t t) {
    if (t >= c.first_silent) return kWcSilent;
    if (t >= 2 && t < 2 + c.interior) return kWcInterior;
    return kWcEdge;
}
// edge frames of a clip, in frame order: their number (<= kWcMaxEdges) and the frame of the k-th one -- frames 0 and 1 below first_silent,
// then the frames from 2 + interior up to first_silent
MS_WC_HD unsigned wc_edge_count(const WcClip &c) {
    const uint64_t head = c.first_silent < 2 ? c.first_silent : 2;
    uint64_t tail = c.first_silent > 2 + c.interior ? c.first_silent - (2 + c.interior) : 0;
    if (tail > kWcMaxEdges - head) tail = kWcMaxEdges - head;
    return static_cast<unsigned>(head + tail);
}
MS_WC_HD uint64_t wc_edge_frame(const WcClip &c, unsigned k) {
    const uint64_t head = c.first_silent < 2 ? c.first_silent : 2;
    return k < head ? k : 2 + c.interior + (k - head);
}
MS_WC_HD unsigned wc_edges(const WcClip &c, uint64_t (&t_of)[kWcMaxEdges]) {
    const unsigned n = wc_edge_count(c);
    for (unsigned k = 0; k < n; ++k) t_of[k] = wc_edge_frame(c, k);
    return n;
}
// sample i (0 .. 399) of frame t: the index into the clip it is read from, or -1: a zero of the extension.  The rule of the gather kernel.
MS_WC_HD int64_t wc_source_index(const WcClip &c, uint64_t t, unsigned i) {
    int64_t idx = static_cast<int64_t>(t * kWcHop + i) - static_cast<int64_t>(kWcPad);
    if (idx < 0) idx = -idx;
    if (idx >= static_cast<int64_t>(c.P)) idx = 2 * (static_cast<int64_t>(c.P) - 1) - idx;
    return idx < static_cast<int64_t>(c.n_eff) ? idx : -1;
}

// ---- the device tables of a batch ------------------------------------------------------------------------------------------------------
struct WcEdge {              // one edge frame: what the gather kernel reads (48 bytes)
    uint64_t pcm_off;        // first sample of the clip
    uint64_t n_eff, P, t;
    uint64_t row_off;        // first float of the frame's raw row
    uint64_t clip;
};
struct WcRecord {            // one clip: what the fill and finalise passes read (32 bytes)
    uint64_t rows_off;       // first float of the clip's raw rows [T][n_mels]
    uint64_t out_off;        // first float of the clip's output
    uint64_t T, first_silent;
};
struct WcBatch {
    std::vector<WcClip> clips;
    // the interior as a plain ragged batch of un-centred frames: offsets + 120 samples, interior counts, outputs two rows in
    std::vector<uint64_t> in_off, in_frames, in_out_off;
    std::vector<WcEdge> edges;
    std::vector<WcRecord> records;
    uint64_t total_frames = 0, interior_frames = 0, silent_frames = 0, max_T = 0;
    uint64_t rows_floats = 0;       // of the packed raw rows (what the scratch of the normalised call holds)
};
// h_off == nullptr: uniform, clip i starts at i * clip_stride and is lengths[0] long.  rows_off: where each clip's raw rows start
// (nullptr: packed in clip order); out_off: the same for the normalised output.
inline WcBatch wc_plan(const uint64_t *h_off, const uint64_t *lengths, uint64_t clip_stride, uint32_t n_clips, uint64_t pad_to, int n_mels,
                       const uint64_t *rows_off, const uint64_t *out_off) {
    WcBatch b;
    const uint64_t nm = static_cast<uint64_t>(n_mels);
    b.clips.resize(n_clips); b.in_off.resize(n_clips); b.in_frames.resize(n_clips); b.in_out_off.resize(n_clips); b.records.resize(n_clips);
    uint64_t cursor = 0;
    for (uint32_t i = 0; i < n_clips; ++i) {
        const uint64_t off = h_off ? h_off[i] : i * clip_stride, n = h_off ? lengths[i] : lengths[0];
        const WcClip c = wc_clip(n, pad_to);
        b.clips[i] = c;
        const uint64_t ro = rows_off ? rows_off[i] : cursor, oo = out_off ? out_off[i] : cursor;
        b.in_off[i] = off + kWcShift;
        b.in_frames[i] = c.interior;
        b.in_out_off[i] = ro + 2 * nm;
        b.records[i] = WcRecord{ro, oo, c.T, c.first_silent};
        uint64_t te[kWcMaxEdges];
        const unsigned ne = wc_edges(c, te);
        for (unsigned k = 0; k < ne; ++k) b.edges.push_back(WcEdge{off, c.n_eff, c.P, te[k], ro + te[k] * nm, i});
        cursor += c.T * nm;
        b.total_frames += c.T; b.interior_frames += c.interior; b.silent_frames += c.T - c.first_silent;
        if (c.T > b.max_T) b.max_T = c.T;
    }
    b.rows_floats = cursor;
    return b;
}

// ---- the arguments -------------------------------------------------------------------------------------------------------------------------
// kWcSlots: nothing to compute, but the clips' maximum slots (split calls) are to be set to -10 -- no clip has a frame
enum WcVerdict { kWcGo = 0, kWcDone = 1, kWcSlots = 2, kWcFail = 3 };
struct WcArgs {
    WcVerdict verdict;
    int status;
    const char *msg;
};
constexpr bool wc_pad_ok(uint64_t pad_to) { return pad_to == 0 || pad_to >= kWcFft; }
// In this order: the context, its support, pad_to, no clips, (ragged) the tables, (uniform) the stride, no frame at all, the device
// pointers, (split) d_clip_max.  total_frames: of the whole batch (the caller counts them only when the tables are there).
inline WcArgs wc_args(bool have_ctx, bool supported, uint64_t pad_to, bool ragged, uint32_t n_clips, const void *h_offsets, const void *h_lengths,
                      uint64_t clip_stride, uint64_t clip_len, uint64_t total_frames, const void *pcm, const void *rows, bool split, const void *clip_max) {
    if (!have_ctx) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "ctx is NULL"};
    if (!supported) return {kWcFail, MELSPEC_ERR_UNSUPPORTED, nullptr};
    if (!wc_pad_ok(pad_to)) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "pad_to must be 0 or at least 400"};
    if (n_clips == 0) return {kWcDone, MELSPEC_OK, nullptr};
    if (ragged && (!h_offsets || !h_lengths)) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL"};
    if (!ragged && n_clips > 1 && clip_stride < clip_len && clip_stride != 0) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "clip_stride smaller than clip_len"};
    if (total_frames == 0) return {split && clip_max ? kWcSlots : kWcDone, MELSPEC_OK, nullptr};
    if (!pcm || !rows) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"};
    if (split && !clip_max) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "d_clip_max is NULL"};
    return {kWcGo, MELSPEC_OK, nullptr};
}

// ---- 16-bit ends (melspec_whisper_*_io): int16 PCM in, f16 / bf16 out --------------------------------------------------------------------
// Every offset, stride and length above counts ELEMENTS of the call's sample / row type, so the plans do not change; what is new is the
// size of an element, the alignment a device pointer needs, and when a mel-major tile of the finalise pass may leave as 16-byte stores.
constexpr bool wc_pcm_known(int t) { return t == MELSPEC_PCM_F32 || t == MELSPEC_PCM_S16; }
constexpr bool wc_out_known(int t) { return t == MELSPEC_OUT_F32 || t == MELSPEC_OUT_F16 || t == MELSPEC_OUT_BF16; }
constexpr size_t wc_pcm_bytes(int t) { return t == MELSPEC_PCM_S16 ? 2 : 4; }
constexpr size_t wc_out_bytes(int t) { return t == MELSPEC_OUT_F32 ? 4 : 2; }
// natural alignment of the element types, nothing more: a clip may start at an odd int16 sample, an output at an odd 16-bit element
inline bool wc_io_misaligned(const void *pcm, int pcm_dtype, const void *dst, int out_dtype) {
    return (reinterpret_cast<uintptr_t>(pcm) & (wc_pcm_bytes(pcm_dtype) - 1)) != 0 || (reinterpret_cast<uintptr_t>(dst) & (wc_out_bytes(out_dtype) - 1)) != 0;
}
// A full mel-major tile of clip (T frames, output at element out_off of the array at address out_addr) leaves as 16-byte stores of
// 16 / elem_bytes values: piece q of mel row m starts at element out_off + m T + 64 tile + (16 / elem_bytes) q, a multiple of
// 16 / elem_bytes when T and out_off are, on a 16-byte aligned base.  Anything else goes element by element -- no wider store ever goes
// to an address whose alignment is not proven here.
constexpr bool wc_wide_ok(uint64_t T, uint64_t out_off, uintptr_t out_addr, size_t elem_bytes) {
    return ((T | out_off) & (16 / elem_bytes - 1)) == 0 && (out_addr & 15) == 0;
}
// wc_args with the dtype codes in front (right after the NULL context) and the alignment of the device pointers behind their NULL checks;
// (F32, F32) is wc_args itself
inline WcArgs wc_args_io(bool have_ctx, bool supported, int pcm_dtype, int out_dtype, uint64_t pad_to, bool ragged, uint32_t n_clips, const void *h_offsets,
                         const void *h_lengths, uint64_t clip_stride, uint64_t clip_len, uint64_t total_frames, const void *pcm, const void *rows, bool split,
                         const void *clip_max) {
    if (!have_ctx) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "ctx is NULL"};
    if (!wc_pcm_known(pcm_dtype)) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16"};
    if (!wc_out_known(out_dtype)) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "out_dtype must be MELSPEC_OUT_F32, MELSPEC_OUT_F16 or MELSPEC_OUT_BF16"};
    const WcArgs a = wc_args(have_ctx, supported, pad_to, ragged, n_clips, h_offsets, h_lengths, clip_stride, clip_len, total_frames, pcm, rows, split, clip_max);
    if (a.verdict == kWcGo && (pcm_dtype != MELSPEC_PCM_F32 || out_dtype != MELSPEC_OUT_F32) && wc_io_misaligned(pcm, pcm_dtype, rows, out_dtype))
        return {kWcFail, MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type"};
    return a;
}

// ---- the clip table in device memory (melspec_whisper_compute_ragged_device_desc*) ---------------------------------------------------------
// pad_to >= 400 is required, so every clip has T = pad_to / 160 frames and the packed offsets are i * T * n_mels: what the host cannot know
// is each clip's classes.  One workgroup of kWcDescThreads threads plans the batch (wc_plan_desc_kernel, whisper_desc_kernels.hpp); thread
// tid owns the clips of wc_desc_slice, counts their edge frames (wc_desc_count), and once the counts in front of it are summed writes
// its clips' entries (wc_desc_write); the entries that do not depend on the table are written for the whole capacity (wc_desc_fixed).
// The functions are the kernel's text; tests/cpp/whisper_desc_plan_host.cpp runs them serially for 1024 "threads" against wc_plan.
//
// The plan buffer (wc_desc_bytes), every array 8-byte aligned, cap = kWcMaxEdges * n_clips edge slots:
//   rec [n]                    WcRecord, what the fill / finalise passes read
//   in_off, in_len, in_out_off [n] u64: the interior as a ragged batch of un-centred frames for plan_ragged_device_kernel -- clip start
//                              offset + 120, length 400 + 160 (interior - 1) samples or 0, rows two rows in
//   edges [cap]                WcEdge, compacted in clip order; entries at and past *n_edges are not written and not read
//   e_off, e_frames, e_out_off [cap], e_prefix [cap + 1], 4 spare words (the look-ahead of locate_unit): the edge launch's batch, one
//                              "clip" of one frame per edge -- e_off = 400 e, e_frames = 1, e_prefix = e for the whole capacity;
//                              e_out_off [e] = the frame's row, written for e < *n_edges only
//   n_edges                    u64, the true count: BatchDesc::d_n_units of the edge launch, the gather kernel's bound
//   e_blk [cap / 16 + 1]       u32 = 16 k;  e_map [cap] u32: the clip (maximum word) of edge e, written for e < *n_edges only
constexpr uint32_t kWcDescThreads = 1024;
constexpr uint32_t kWcDescUnitBlock = 16;                          // kUnitBlock
constexpr uint32_t kWcDescMaxClips = 0xffffffffu / kWcMaxEdges;    // the edge slots are counted in 32 bits

struct WcDescIn {
    const uint64_t *off, *len;              // the caller's tables
    const uint64_t *rows_off, *out_off;     // either may be null: packed in clip order (wc_plan's arguments)
    uint32_t n_clips, n_mels;
    uint64_t pad_to;
};
struct WcDescTables {
    WcRecord *rec;
    uint64_t *in_off, *in_len, *in_out_off;
    WcEdge *edges;
    uint64_t *e_off, *e_frames, *e_out_off, *e_prefix, *n_edges;
    uint32_t *e_blk, *e_map;
};
MS_WC_HD uint64_t wc_desc_cap(uint32_t n_clips) { return kWcMaxEdges * static_cast<uint64_t>(n_clips); }
MS_WC_HD uint64_t wc_desc_blocks(uint32_t n_clips) { return wc_desc_cap(n_clips) / kWcDescUnitBlock + 1; }
MS_WC_HD size_t wc_desc_bytes(uint32_t n_clips) {
    const size_t n = n_clips, cap = static_cast<size_t>(wc_desc_cap(n_clips));
    const size_t b = n * sizeof(WcRecord) + 3 * n * sizeof(uint64_t) + cap * sizeof(WcEdge) + (4 * cap + 1 + 4 + 1) * sizeof(uint64_t) +
                     (static_cast<size_t>(wc_desc_blocks(n_clips)) + cap) * sizeof(uint32_t);
    return (b + 15) & ~static_cast<size_t>(15);
}
MS_WC_HD WcDescTables wc_desc_tables(void *buf, uint32_t n_clips) {
    WcDescTables t;
    const size_t n = n_clips, cap = static_cast<size_t>(wc_desc_cap(n_clips));
    t.rec = static_cast<WcRecord *>(buf);
    t.in_off = reinterpret_cast<uint64_t *>(t.rec + n); t.in_len = t.in_off + n; t.in_out_off = t.in_len + n;
    t.edges = reinterpret_cast<WcEdge *>(t.in_out_off + n);
    t.e_off = reinterpret_cast<uint64_t *>(t.edges + cap); t.e_frames = t.e_off + cap; t.e_out_off = t.e_frames + cap; t.e_prefix = t.e_out_off + cap;
    t.n_edges = t.e_prefix + cap + 1 + 4;
    t.e_blk = reinterpret_cast<uint32_t *>(t.n_edges + 1); t.e_map = t.e_blk + wc_desc_blocks(n_clips);
    return t;
}
// the interior of a clip as a length the un-centred frame count recovers: frames(n) = n < 400 ? 0 : (n - 400) / 160 + 1
MS_WC_HD uint64_t wc_interior_len(const WcClip &c) { return c.interior ? kWcFft + kWcHop * (c.interior - 1) : 0; }
// what the host sizes the interior launch from: every clip has at most T - 2 interior frames
MS_WC_HD uint64_t wc_desc_interior_bound(uint32_t n_clips, uint64_t pad_to) {
    const uint64_t T = pad_to / kWcHop;
    return static_cast<uint64_t>(n_clips) * (T > 2 ? T - 2 : 0);
}

// the clips of thread tid: a contiguous slice, [c0, c1) (tid * per in 32 bits would wrap for n_clips near 2^32)
MS_WC_HD void wc_desc_slice(uint32_t n_clips, uint32_t tid, uint32_t &c0, uint32_t &c1) {
    const uint32_t per = n_clips / kWcDescThreads + (n_clips % kWcDescThreads != 0);
    const uint64_t b0 = static_cast<uint64_t>(tid) * per;
    c0 = b0 < n_clips ? static_cast<uint32_t>(b0) : n_clips;
    c1 = b0 + per < n_clips ? static_cast<uint32_t>(b0 + per) : n_clips;
}
MS_WC_HD uint64_t wc_desc_count(const WcDescIn &q, uint32_t c0, uint32_t c1) {
    uint64_t edges = 0;
    for (uint32_t c = c0; c < c1; ++c) edges += wc_edge_count(wc_clip(q.len[c], q.pad_to));
    return edges;
}
// first_edge: the edge frames of the clips in front of c0
MS_WC_HD void wc_desc_write(const WcDescIn &q, const WcDescTables &t, uint32_t c0, uint32_t c1, uint64_t first_edge) {
    const uint64_t nm = q.n_mels;
    for (uint32_t c = c0; c < c1; ++c) {
        const uint64_t off = q.off[c];
        const WcClip k = wc_clip(q.len[c], q.pad_to);
        const uint64_t cursor = static_cast<uint64_t>(c) * k.T * nm;
        const uint64_t ro = q.rows_off ? q.rows_off[c] : cursor, oo = q.out_off ? q.out_off[c] : cursor;
        t.rec[c] = WcRecord{ro, oo, k.T, k.first_silent};
        t.in_off[c] = off + kWcShift; t.in_len[c] = wc_interior_len(k); t.in_out_off[c] = ro + 2 * nm;
        const unsigned ne = wc_edge_count(k);
        for (unsigned j = 0; j < ne; ++j, ++first_edge) {
            const uint64_t te = wc_edge_frame(k, j);
            t.edges[first_edge] = WcEdge{off, k.n_eff, k.P, te, ro + te * nm, c};
            t.e_out_off[first_edge] = ro + te * nm;
            t.e_map[first_edge] = c;
        }
    }
}
// the entries that are the same for every table, slots tid, tid + kWcDescThreads, ... of the capacity
MS_WC_HD void wc_desc_fixed(const WcDescTables &t, uint32_t n_clips, uint32_t tid) {
    const uint64_t cap = wc_desc_cap(n_clips), blocks = wc_desc_blocks(n_clips);
    for (uint64_t e = tid; e < cap; e += kWcDescThreads) { t.e_off[e] = e * kWcFft; t.e_frames[e] = 1; t.e_prefix[e] = e; }
    for (uint64_t e = cap + tid; e < cap + 1 + 4; e += kWcDescThreads) t.e_prefix[e] = cap;
    for (uint64_t b = tid; b < blocks; b += kWcDescThreads) t.e_blk[b] = static_cast<uint32_t>(b * kWcDescUnitBlock);
}

// The arguments of the _desc calls, in this order: the context, (io) the dtype codes, its support, pad_to -- which must be a fixed width
// here --, no clips, the tables, the device pointers, (split) d_clip_max, (io) the alignment to the element type, the clip count.  No
// verdict depends on the table's contents: the host never reads it.
inline WcArgs wc_args_desc_io(bool have_ctx, bool supported, bool io, int pcm_dtype, int out_dtype, uint64_t pad_to, uint32_t n_clips, const void *d_offsets,
                              const void *d_lengths, const void *pcm, const void *dst, bool split, const void *clip_max) {
    if (!have_ctx) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "ctx is NULL"};
    if (io && !wc_pcm_known(pcm_dtype)) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16"};
    if (io && !wc_out_known(out_dtype)) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "out_dtype must be MELSPEC_OUT_F32, MELSPEC_OUT_F16 or MELSPEC_OUT_BF16"};
    if (!supported) return {kWcFail, MELSPEC_ERR_UNSUPPORTED, nullptr};
    if (pad_to == 0)
        return {kWcFail, MELSPEC_ERR_INVALID_ARG, "pad_to must be at least 400 with a device-resident clip table: without a fixed width the frame counts are known on the device only"};
    if (pad_to < kWcFft) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "pad_to must be at least 400"};
    if (n_clips == 0) return {kWcDone, MELSPEC_OK, nullptr};
    if (!d_offsets || !d_lengths) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL"};
    if (!pcm || !dst) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"};
    if (split && !clip_max) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "d_clip_max is NULL"};
    if (io && (pcm_dtype != MELSPEC_PCM_F32 || out_dtype != MELSPEC_OUT_F32) && wc_io_misaligned(pcm, pcm_dtype, dst, out_dtype))
        return {kWcFail, MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type"};
    if (n_clips > kWcDescMaxClips) return {kWcFail, MELSPEC_ERR_INVALID_ARG, "too many clips for one call"};
    return {kWcGo, MELSPEC_OK, nullptr};
}
inline WcArgs wc_args_desc(bool have_ctx, bool supported, uint64_t pad_to, uint32_t n_clips, const void *d_offsets, const void *d_lengths, const void *pcm,
                           const void *dst, bool split, const void *clip_max) {
    return wc_args_desc_io(have_ctx, supported, false, MELSPEC_PCM_F32, MELSPEC_OUT_F32, pad_to, n_clips, d_offsets, d_lengths, pcm, dst, split, clip_max);
}

}  // namespace host
}  // namespace melspec
