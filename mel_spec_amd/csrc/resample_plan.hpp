// resample_plan.hpp -- the side of the polyphase resampler (melspec_resample_*, resample.hip) that is arithmetic only: the geometry of a
// rate pair, the tap table in f64, the clip table a call sends to the device and the tile arithmetic of the kernel.  Nothing from HIP in
// here but the host-device qualifier: tests/cpp/resample_plan_host.cpp builds it on the host, with and without sanitizers.
//
// The filter is torchaudio.functional.resample's default (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99), stated with integer
// arguments (include/melspec_resample.h has the whole definition):
//   g = gcd(rate_in, rate_out), orig = rate_in / g, new = rate_out / g, M = max(orig, new), m_ = min(orig, new)
//   width = ceil(600 orig / (99 m_)), K = 2 width + orig
//   phase p in [0, new), tap k in [0, K): m = (k - width) new - p orig; inside iff 99 |m| < 600 M, outside taps are exactly 0
//   t = (99.0 m) / (100.0 M);  h[p][k] = sinc(pi t) cos^2(pi t / 12) (99.0 m_) / (100.0 orig)
//   y[j new + p] = sum_k h[p][k] x[j orig + k - width], x zero outside [0, L), out_len = ceil(new L / orig)
// The inside taps of a phase are contiguous: [first, first + count).  The kernel reads, for every phase, a window of `taps` = the largest
// count of any phase, [start, start + taps) with start = min(first, K - taps): the window stays inside the dense one and its padding is
// exact zeros.
//
// A tile is kBlocks consecutive output blocks (of `new` outputs each) of one clip, j0 .. j0 + nb - 1; it reads the samples
// [j0 orig - width, (j0 + nb) orig + width) of its clip, staged with zeros outside [0, L).  A call's table has one record per clip and the
// number of tiles in front of it; a workgroup finds the clip of tile t by bisection.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/melspec_hip.h"

#if defined(__HIPCC__)
#define MS_RS_HD __host__ __device__ inline
#else
#define MS_RS_HD inline
#endif

namespace melspec {
namespace host {

constexpr uint32_t kRsMaxRatio = 4096;          // the largest reduced orig / new
constexpr uint32_t kRsThreads = 256;
constexpr uint32_t kRsTileOutputs = 1024;       // outputs a tile aims at
constexpr size_t kRsLdsBudget = 64 * 1024;      // of one workgroup: the default limit of a launch's dynamic LDS, two workgroups per CU at least

struct RsGeom {
    uint32_t orig = 0, nw = 0, width = 0, K = 0;
    uint32_t taps = 0;           // max_inside_taps
    uint64_t M = 0, m_ = 0;
    bool copy = false;           // rate_in == rate_out: no filter
};

inline uint32_t rs_gcd(uint32_t a, uint32_t b) {
    while (b) { const uint32_t t = a % b; a = b; b = t; }
    return a;
}
inline int64_t rs_floor_div(int64_t a, int64_t b) { return a / b - ((a % b != 0 && (a % b < 0) != (b < 0)) ? 1 : 0); }
inline int64_t rs_ceil_div(int64_t a, int64_t b) { return -rs_floor_div(-a, b); }

MS_RS_HD int64_t rs_m(uint32_t orig, uint32_t nw, uint32_t width, uint32_t p, uint32_t k) {
    return (static_cast<int64_t>(k) - width) * nw - static_cast<int64_t>(p) * orig;
}
MS_RS_HD bool rs_inside(int64_t m, uint64_t M) { return 99 * static_cast<uint64_t>(m < 0 ? -m : m) < 600 * M; }

// the inside taps of phase p: [first, first + count)
inline void rs_inside_range(const RsGeom &g, uint32_t p, uint32_t &first, uint32_t &count) {
    const int64_t R = static_cast<int64_t>((600 * g.M - 1) / 99);         // inside iff |m| <= R
    const int64_t c = static_cast<int64_t>(p) * g.orig;
    int64_t lo = rs_ceil_div(c - R, g.nw) + g.width, hi = rs_floor_div(c + R, g.nw) + g.width;      // k in [lo, hi]
    if (lo < 0) lo = 0;
    if (hi > static_cast<int64_t>(g.K) - 1) hi = static_cast<int64_t>(g.K) - 1;
    first = static_cast<uint32_t>(lo);
    count = hi >= lo ? static_cast<uint32_t>(hi - lo + 1) : 0;
}

// MELSPEC_OK, or the status of a pair the resampler does not take
inline int rs_geometry(uint32_t rate_in, uint32_t rate_out, RsGeom &g) {
    if (rate_in == 0 || rate_out == 0) return MELSPEC_ERR_INVALID_ARG;
    const uint32_t d = rs_gcd(rate_in, rate_out);
    g.orig = rate_in / d; g.nw = rate_out / d;
    if (g.orig > kRsMaxRatio || g.nw > kRsMaxRatio) return MELSPEC_ERR_UNSUPPORTED;
    g.M = g.orig > g.nw ? g.orig : g.nw;
    g.m_ = g.orig < g.nw ? g.orig : g.nw;
    g.width = static_cast<uint32_t>((600ull * g.orig + 99 * g.m_ - 1) / (99 * g.m_));
    g.K = 2 * g.width + g.orig;
    g.copy = rate_in == rate_out;
    g.taps = 0;
    for (uint32_t p = 0; p < g.nw; ++p) {
        uint32_t f, c;
        rs_inside_range(g, p, f, c);
        if (c > g.taps) g.taps = c;
    }
    return MELSPEC_OK;
}

inline double rs_tap(const RsGeom &g, uint32_t p, uint32_t k) {
    const int64_t m = rs_m(g.orig, g.nw, g.width, p, k);
    if (!rs_inside(m, g.M)) return 0.0;
    const double pi = 3.14159265358979323846;
    const double t = (99.0 * static_cast<double>(m)) / (100.0 * static_cast<double>(g.M));
    const double a = pi * t;
    const double s = m == 0 ? 1.0 : std::sin(a) / a;
    const double c = std::cos(a / 12.0);
    return s * (c * c) * ((99.0 * static_cast<double>(g.m_)) / (100.0 * static_cast<double>(g.orig)));
}

// the dense table, [new][K]
inline void rs_dense_taps(const RsGeom &g, double *taps) {
    for (uint32_t p = 0; p < g.nw; ++p)
        for (uint32_t k = 0; k < g.K; ++k) taps[static_cast<size_t>(p) * g.K + k] = rs_tap(g, p, k);
}

// what the kernel reads: start[p] (the first tap of phase p's window) and the windows tap-major, win[t * new + p] = h[p][start[p] + t],
// so that consecutive lanes (consecutive phases) read consecutive words
struct RsTable {
    std::vector<uint32_t> start;
    std::vector<double> win;
};
inline RsTable rs_table(const RsGeom &g) {
    RsTable tb;
    tb.start.resize(g.nw);
    tb.win.resize(static_cast<size_t>(g.taps) * g.nw);
    for (uint32_t p = 0; p < g.nw; ++p) {
        uint32_t f, c;
        rs_inside_range(g, p, f, c);
        const uint32_t s = f + g.taps <= g.K ? f : g.K - g.taps;
        tb.start[p] = s;
        for (uint32_t t = 0; t < g.taps; ++t) tb.win[static_cast<size_t>(t) * g.nw + p] = rs_tap(g, p, s + t);
    }
    return tb;
}

MS_RS_HD uint64_t rs_out_len(uint32_t orig, uint32_t nw, uint64_t n_in) {
    // ceil(new n / orig) without the product's overflow: n = q orig + r
    const uint64_t q = n_in / orig, r = n_in % orig;
    return q * nw + (r * nw + orig - 1) / orig;
}

// ---- tiles ----
// how the kernel runs a geometry: where the samples and the taps are read from, and the blocks of a tile
enum RsMode { kRsLdsAll = 0, kRsLdsSamples = 1, kRsGlobal = 2, kRsCopy = 3 };
struct RsLaunch {
    int mode = kRsLdsAll;
    uint32_t blocks = 1;         // output blocks per tile (kRsCopy: kRsTileOutputs samples per tile, orig = new = 1)
    size_t lds = 0;              // bytes of dynamic LDS
};
MS_RS_HD uint64_t rs_span(uint32_t orig, uint32_t width, uint32_t blocks) { return static_cast<uint64_t>(blocks) * orig + 2ull * width; }
inline RsLaunch rs_launch(const RsGeom &g) {
    RsLaunch l;
    if (g.copy) { l.mode = kRsCopy; l.blocks = kRsTileOutputs; return l; }
    const size_t tab = static_cast<size_t>(g.taps) * g.nw * 8 + static_cast<size_t>(g.nw) * 4 + 8;
    l.blocks = kRsTileOutputs / g.nw ? kRsTileOutputs / g.nw : 1;
    if (rs_span(g.orig, g.width, 1) * 8 > kRsLdsBudget) { l.mode = kRsGlobal; l.lds = 0; return l; }
    const bool tab_fits = tab + rs_span(g.orig, g.width, 1) * 8 <= kRsLdsBudget;
    const size_t room = tab_fits ? kRsLdsBudget - tab : kRsLdsBudget;
    while (l.blocks > 1 && rs_span(g.orig, g.width, l.blocks) * 8 > room) --l.blocks;
    l.mode = tab_fits ? kRsLdsAll : kRsLdsSamples;
    l.lds = rs_span(g.orig, g.width, l.blocks) * 8 + (tab_fits ? tab : 0);
    return l;
}

// one record per clip, and one more behind the last whose tile0 is the call's number of tiles
struct RsClip {
    uint64_t in_off;     // of the clip's first sample, in elements
    uint64_t len;        // samples
    uint64_t out_off;    // of the clip's first output, in elements
    uint64_t tile0;      // tiles in front of this clip
};
MS_RS_HD uint64_t rs_clip_tiles(uint32_t orig, uint32_t nw, uint32_t blocks, uint64_t len) {
    const uint64_t n = rs_out_len(orig, nw, len), per = static_cast<uint64_t>(blocks) * nw;
    return n / per + (n % per ? 1 : 0);
}
// the clip of tile t: the last record with tile0 <= t (clips without a tile share their tile0 with the next one)
MS_RS_HD uint32_t rs_find_clip(const RsClip *tab, uint32_t n_clips, uint64_t t) {
    uint32_t lo = 0, hi = n_clips;           // tab[lo].tile0 <= t < tab[hi].tile0
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (tab[mid].tile0 <= t) lo = mid; else hi = mid;
    }
    return lo;
}
// tile t of a clip (t counted inside the clip): its first block, its outputs [o0, o0 + n_out) and the samples it stages, [s0, s0 + span) in
// the clip's coordinates (s0 may be negative), of which [lo, hi) are inside the clip
struct RsTile {
    uint64_t j0, o0;
    uint32_t n_out;
    int64_t s0;
    uint32_t span, lo, hi;      // lo, hi relative to s0
};
MS_RS_HD RsTile rs_tile(uint32_t orig, uint32_t nw, uint32_t width, uint32_t blocks, uint64_t len, uint64_t t) {
    RsTile tl;
    const uint64_t n = rs_out_len(orig, nw, len), per = static_cast<uint64_t>(blocks) * nw;
    tl.j0 = t * blocks;
    tl.o0 = t * per;
    tl.n_out = static_cast<uint32_t>(n - tl.o0 < per ? n - tl.o0 : per);
    tl.s0 = static_cast<int64_t>(tl.j0 * orig) - static_cast<int64_t>(width);
    tl.span = static_cast<uint32_t>(rs_span(orig, width, blocks));
    const int64_t e = tl.s0 + static_cast<int64_t>(tl.span);
    const int64_t a = tl.s0 < 0 ? 0 : tl.s0, b = e < static_cast<int64_t>(len) ? e : static_cast<int64_t>(len);
    tl.lo = static_cast<uint32_t>(a - tl.s0);
    tl.hi = b > a ? static_cast<uint32_t>(b - tl.s0) : tl.lo;
    return tl;
}

// the table of a ragged (offsets != NULL) or uniform batch; returns the number of tiles
inline uint64_t rs_plan(const RsGeom &g, const RsLaunch &l, const uint64_t *offsets, const uint64_t *lengths, const uint64_t *out_offsets,
                        uint64_t clip_stride, uint64_t clip_len, uint64_t out_stride, uint32_t n_clips, RsClip *tab) {
    uint64_t tiles = 0, cursor = 0;
    for (uint32_t i = 0; i < n_clips; ++i) {
        const uint64_t len = offsets ? lengths[i] : clip_len;
        RsClip &c = tab[i];
        c.in_off = offsets ? offsets[i] : clip_stride * i;
        c.len = len;
        c.out_off = offsets ? (out_offsets ? out_offsets[i] : cursor) : out_stride * i;
        c.tile0 = tiles;
        tiles += rs_clip_tiles(g.orig, g.nw, l.blocks, len);
        cursor += rs_out_len(g.orig, g.nw, len);
    }
    tab[n_clips] = RsClip{0, 0, 0, tiles};
    return tiles;
}

// ---- the calls' arguments, in the order the header states ----
inline bool rs_dtype_known(int t) { return t == MELSPEC_PCM_F32 || t == MELSPEC_PCM_S16; }
inline bool rs_misaligned(const void *pcm, int pcm_dtype, const void *out) {
    return (reinterpret_cast<uintptr_t>(pcm) & (pcm_dtype == MELSPEC_PCM_S16 ? 1u : 3u)) || (reinterpret_cast<uintptr_t>(out) & 3u);
}

}  // namespace host
}  // namespace melspec
