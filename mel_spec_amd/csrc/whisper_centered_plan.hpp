// whisper_centered_plan.hpp -- the host side of the centred Whisper features (melspec_whisper_*, whisper_centered.hip) that is arithmetic
// only: the frame count of a clip, the class of every frame (interior / edge / silent), the interior of a batch as a plain ragged batch for
// the existing planners, the list of edge frames, the per-clip records of the fill / finalise passes, and the checks of the calls'
// arguments in their order; for the calls with int16 PCM in / f16, bf16 out (melspec_whisper_*_io) the element sizes, the alignment rule
// and the 16-byte store rule of the finalise pass.  Nothing from HIP in here: tests/cpp/whisper_centered_host.cpp and
// tests/cpp/whisper_centered_io_host.cpp build it on the host, with and without sanitizers.
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

inline WcClip wc_clip(uint64_t n, uint64_t pad_to) {
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
inline WcClass wc_class(const WcClip &c, uint64_t t) {
    if (t >= c.first_silent) return kWcSilent;
    if (t >= 2 && t < 2 + c.interior) return kWcInterior;
    return kWcEdge;
}
// edge frames of a clip, in frame order; returns their number (<= kWcMaxEdges)
inline unsigned wc_edges(const WcClip &c, uint64_t (&t_of)[kWcMaxEdges]) {
    unsigned k = 0;
    for (uint64_t t = 0; t < 2 && t < c.first_silent; ++t) t_of[k++] = t;
    for (uint64_t t = 2 + c.interior; t < c.first_silent && k < kWcMaxEdges; ++t) t_of[k++] = t;
    return k;
}
// sample i (0 .. 399) of frame t: the index into the clip it is read from, or -1: a zero of the extension.  The rule of the gather kernel.
inline int64_t wc_source_index(const WcClip &c, uint64_t t, unsigned i) {
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

}  // namespace host
}  // namespace melspec
