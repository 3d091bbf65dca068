// resample_plan_host.cpp -- the side of the polyphase resampler (melspec_resample_*) that is arithmetic only
// (mel_spec_amd/csrc/resample_plan.hpp): the geometry and the per-phase inside ranges against brute force for nine rate pairs, the
// kernel's tap windows against the dense table, and the tiles -- every output covered exactly once, every staged span holding every
// sample of its outputs' windows, no read outside [0, L) -- for clip lengths around every edge, and again with clip offsets and lengths
// near 2^40 (the 64-bit index arithmetic, without touching memory).  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/resample_plan_host.cpp -o /tmp/resample_plan_host && /tmp/resample_plan_host
#include <cstdio>
#include <vector>

#include "resample_plan.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

typedef unsigned long long ull;

static const struct { uint32_t in, out, orig, nw, width, K, taps_lo, taps_hi; } kPairs[] = {
    {48000, 16000, 3, 1, 19, 41, 37, 37},   {44100, 16000, 441, 160, 17, 475, 33, 34}, {8000, 16000, 1, 2, 7, 15, 12, 13},
    {22050, 16000, 441, 320, 9, 459, 16, 17}, {24000, 16000, 3, 2, 10, 23, 18, 19},   {32000, 16000, 2, 1, 13, 28, 0, 0},
    {11025, 16000, 441, 640, 7, 455, 0, 0},  {96000, 16000, 6, 1, 37, 80, 0, 0},      {16000, 24000, 2, 3, 7, 16, 0, 0}};

// the tiles of one clip of len samples whose record sits at in_off / out_off: coverage, spans, reads
static void check_clip(const RsGeom &g, const RsLaunch &l, const RsTable &tb, uint64_t in_off, uint64_t len, uint64_t out_off, bool every_output) {
    const uint64_t n_out = rs_out_len(g.orig, g.nw, len);
    const uint64_t tiles = rs_clip_tiles(g.orig, g.nw, l.blocks, len);
    uint64_t next = 0;
    for (uint64_t t = 0; t < tiles; ++t) {
        const RsTile tl = rs_tile(g.orig, g.nw, g.width, l.blocks, len, t);
        CHECK(tl.o0 == next && tl.n_out >= 1 && tl.n_out <= static_cast<uint64_t>(l.blocks) * g.nw, "len %llu tile %llu: outputs [%llu, +%u)", (ull)len, (ull)t, (ull)tl.o0, tl.n_out);
        next = tl.o0 + tl.n_out;
        CHECK(tl.j0 * g.nw == tl.o0 && tl.span == rs_span(g.orig, g.width, l.blocks), "len %llu tile %llu: first block", (ull)len, (ull)t);
        // what is staged from the clip lies inside it; what is not staged from it lies outside (zeros)
        CHECK(tl.lo <= tl.hi && tl.hi <= tl.span, "len %llu tile %llu: lo %u hi %u span %u", (ull)len, (ull)t, tl.lo, tl.hi, tl.span);
        if (tl.hi > tl.lo) {
            CHECK(tl.s0 + tl.lo >= 0 && static_cast<uint64_t>(tl.s0 + tl.hi) <= len, "len %llu tile %llu: a read outside the clip", (ull)len, (ull)t);
            // the addresses of the first and the last element read, in elements: no wrap
            const uint64_t first = in_off + static_cast<uint64_t>(tl.s0 + tl.lo), last = in_off + static_cast<uint64_t>(tl.s0 + tl.hi) - 1;
            CHECK(first >= in_off && last < in_off + len && last >= first, "len %llu tile %llu: addresses", (ull)len, (ull)t);
        }
        if (tl.lo > 0) CHECK(tl.s0 + static_cast<int64_t>(tl.lo) == 0 || tl.hi == tl.lo, "len %llu tile %llu: zeros in front of a sample of the clip", (ull)len, (ull)t);
        if (tl.hi < tl.span && tl.hi > tl.lo) CHECK(static_cast<uint64_t>(tl.s0 + tl.hi) == len, "len %llu tile %llu: zeros over a sample of the clip", (ull)len, (ull)t);
        CHECK(out_off + tl.o0 + tl.n_out <= out_off + n_out && out_off + tl.o0 >= out_off, "len %llu tile %llu: a store past out_len", (ull)len, (ull)t);
        // every output's window: inside the staged span, and equal to what the definition reads
        const uint32_t step = every_output ? 1 : (tl.n_out > 7 ? tl.n_out / 7 : 1);
        for (uint32_t o = 0; o < tl.n_out; o = (o + step < tl.n_out || o == tl.n_out - 1) ? o + step : tl.n_out - 1) {
            const uint32_t jb = o / g.nw, p = o % g.nw;
            const uint32_t base = jb * g.orig + tb.start[p];
            CHECK(static_cast<uint64_t>(base) + g.taps <= tl.span, "len %llu tile %llu output %u: window past the span", (ull)len, (ull)t, o);
            // index in the clip of window tap 0 == (j orig + start - width) of the definition
            const int64_t want = static_cast<int64_t>((tl.j0 + jb) * g.orig) + tb.start[p] - static_cast<int64_t>(g.width);
            CHECK(tl.s0 + static_cast<int64_t>(base) == want, "len %llu tile %llu output %u: window origin", (ull)len, (ull)t, o);
            uint32_t f, c;
            rs_inside_range(g, p, f, c);
            CHECK(tb.start[p] <= f && f + c <= tb.start[p] + g.taps, "phase %u: an inside tap outside the window", p);
        }
    }
    CHECK(next == n_out, "len %llu: outputs covered %llu of %llu", (ull)len, (ull)next, (ull)n_out);
}

int main() {
    for (const auto &pr : kPairs) {
        RsGeom g;
        CHECK(rs_geometry(pr.in, pr.out, g) == MELSPEC_OK, "%u -> %u", pr.in, pr.out);
        CHECK(g.orig == pr.orig && g.nw == pr.nw && g.width == pr.width && g.K == pr.K, "%u -> %u: %u : %u width %u K %u", pr.in, pr.out, g.orig, g.nw, g.width, g.K);
        // ---- inside ranges against brute force ----
        uint32_t lo = ~0u, hi = 0;
        std::vector<double> dense(static_cast<size_t>(g.nw) * g.K);
        rs_dense_taps(g, dense.data());
        for (uint32_t p = 0; p < g.nw; ++p) {
            uint32_t first = 0, count = 0, runs = 0;
            bool in_run = false;
            for (uint32_t k = 0; k < g.K; ++k) {
                const int64_t m = (static_cast<int64_t>(k) - g.width) * g.nw - static_cast<int64_t>(p) * g.orig;
                const bool in = 99 * (m < 0 ? -m : m) < 600 * static_cast<int64_t>(g.M);
                if (in && !in_run) { ++runs; first = k; }
                if (in) ++count;
                in_run = in;
                CHECK((dense[static_cast<size_t>(p) * g.K + k] == 0.0) >= !in, "%u -> %u: an outside tap that is not 0", pr.in, pr.out);
            }
            uint32_t f, c;
            rs_inside_range(g, p, f, c);
            CHECK(runs == 1 && f == first && c == count, "%u -> %u phase %u: inside [%u, +%u), brute force [%u, +%u) in %u runs", pr.in, pr.out, p, f, c, first, count, runs);
            if (count < lo) lo = count;
            if (count > hi) hi = count;
        }
        CHECK(hi == g.taps, "%u -> %u: max_inside_taps %u, brute force %u", pr.in, pr.out, g.taps, hi);
        if (pr.taps_hi) CHECK(lo == pr.taps_lo && hi == pr.taps_hi, "%u -> %u: inside taps %u-%u", pr.in, pr.out, lo, hi);
        // ---- the kernel's windows against the dense table ----
        const RsTable tb = rs_table(g);
        for (uint32_t p = 0; p < g.nw; ++p) {
            CHECK(tb.start[p] + g.taps <= g.K, "%u -> %u phase %u: window past K", pr.in, pr.out, p);
            for (uint32_t k = 0; k < g.K; ++k) {
                const double d = dense[static_cast<size_t>(p) * g.K + k];
                const bool in_win = k >= tb.start[p] && k < tb.start[p] + g.taps;
                if (in_win) CHECK(tb.win[static_cast<size_t>(k - tb.start[p]) * g.nw + p] == d, "%u -> %u phase %u tap %u: window value", pr.in, pr.out, p, k);
                else CHECK(d == 0.0, "%u -> %u phase %u tap %u: a non-zero tap outside the window", pr.in, pr.out, p, k);
            }
        }
        // ---- the launch ----
        const RsLaunch l = rs_launch(g);
        // (11025 -> 16000 has 640 phases of 13 taps, 66.6 KB: its taps stay in their global table)
        const size_t tab_bytes = static_cast<size_t>(g.taps) * g.nw * 8 + g.nw * 4 + 8;
        const int want_mode = pr.in == 11025 ? kRsLdsSamples : kRsLdsAll;
        CHECK(l.mode == want_mode && l.lds <= kRsLdsBudget && l.blocks >= 1, "%u -> %u: mode %d lds %zu", pr.in, pr.out, l.mode, l.lds);
        CHECK(l.lds == rs_span(g.orig, g.width, l.blocks) * 8 + (want_mode == kRsLdsAll ? tab_bytes : 0), "%u -> %u: lds", pr.in, pr.out);
        CHECK(l.blocks == 1 || rs_span(g.orig, g.width, l.blocks + 1) * 8 + (want_mode == kRsLdsAll ? tab_bytes : 0) > kRsLdsBudget || (l.blocks + 1) * g.nw > kRsTileOutputs,
              "%u -> %u: a tile smaller than it has to be", pr.in, pr.out);
        // ---- tiles ----
        const uint64_t tile_in = static_cast<uint64_t>(l.blocks) * g.orig;       // samples whose outputs fill one tile
        const uint64_t lens[] = {0, 1, g.orig, g.width, g.K - 1, g.K + 1, tile_in - 1, tile_in, tile_in + 1, 3 * tile_in + 1};
        for (uint64_t len : lens) {
            check_clip(g, l, tb, 0, len, 0, true);
            CHECK(rs_out_len(g.orig, g.nw, len) == (len * g.nw + g.orig - 1) / g.orig, "%u -> %u: out_len(%llu)", pr.in, pr.out, (ull)len);
        }
        // offsets and lengths near 2^40: first, middle and last tiles through the same checks, a handful of outputs each
        const uint64_t big = (1ull << 40) + 12345;
        for (uint64_t len : {big, big - g.orig + 1}) {
            const uint64_t tiles = rs_clip_tiles(g.orig, g.nw, l.blocks, len), n_out = rs_out_len(g.orig, g.nw, len);
            CHECK(tiles == (n_out + static_cast<uint64_t>(l.blocks) * g.nw - 1) / (static_cast<uint64_t>(l.blocks) * g.nw), "%u -> %u: tiles of 2^40", pr.in, pr.out);
            for (uint64_t t : {uint64_t{0}, tiles / 2, tiles - 2, tiles - 1}) {
                const RsTile tl = rs_tile(g.orig, g.nw, g.width, l.blocks, len, t);
                CHECK(tl.o0 == t * l.blocks * g.nw && tl.o0 + tl.n_out <= n_out && (t + 1 < tiles || tl.o0 + tl.n_out == n_out), "%u -> %u: tile %llu of 2^40", pr.in, pr.out, (ull)t);
                CHECK(tl.s0 == static_cast<int64_t>(t * l.blocks * g.orig) - static_cast<int64_t>(g.width), "%u -> %u: s0 of tile %llu", pr.in, pr.out, (ull)t);
                if (tl.hi > tl.lo) CHECK(tl.s0 + tl.lo >= 0 && static_cast<uint64_t>(tl.s0 + tl.hi) <= len && (big + static_cast<uint64_t>(tl.s0 + tl.hi) - 1) - big < len, "%u -> %u: reads of tile %llu of 2^40", pr.in, pr.out, (ull)t);
                // the last output's window ends inside the span and holds its inside taps
                const uint32_t o = tl.n_out - 1, jb = o / g.nw, p = o % g.nw;
                CHECK(static_cast<uint64_t>(jb) * g.orig + tb.start[p] + g.taps <= tl.span, "%u -> %u: window of tile %llu of 2^40", pr.in, pr.out, (ull)t);
            }
        }
        // ---- the clip table: a ragged batch with empty clips, and the bisection for every tile ----
        {
            const uint64_t lengths[] = {0, tile_in + 1, 0, 0, 1, 3 * tile_in, 0, big, 0};
            const uint64_t offsets[] = {7, big, 9, 9, 11, 13, 15, 2 * big, 3};
            const uint32_t n = 9;
            std::vector<RsClip> tab(n + 1);
            const uint64_t total = rs_plan(g, l, offsets, lengths, nullptr, 0, 0, 0, n, tab.data());
            uint64_t sum = 0, cursor = 0;
            for (uint32_t i = 0; i < n; ++i) {
                CHECK(tab[i].tile0 == sum && tab[i].in_off == offsets[i] && tab[i].len == lengths[i] && tab[i].out_off == cursor, "%u -> %u: record %u", pr.in, pr.out, i);
                sum += rs_clip_tiles(g.orig, g.nw, l.blocks, lengths[i]);
                cursor += rs_out_len(g.orig, g.nw, lengths[i]);
            }
            CHECK(total == sum && tab[n].tile0 == total, "%u -> %u: total tiles", pr.in, pr.out);
            for (uint64_t t : {uint64_t{0}, uint64_t{1}, uint64_t{2}, uint64_t{3}, uint64_t{4}, uint64_t{5}, uint64_t{6}, total / 2, total - 1}) {
                if (t >= total) continue;
                const uint32_t c = rs_find_clip(tab.data(), n, t);
                CHECK(c < n && tab[c].tile0 <= t && t - tab[c].tile0 < rs_clip_tiles(g.orig, g.nw, l.blocks, tab[c].len), "%u -> %u: clip of tile %llu", pr.in, pr.out, (ull)t);
            }
            // uniform: strides
            std::vector<RsClip> u(4);
            const uint64_t ut = rs_plan(g, l, nullptr, nullptr, nullptr, big, tile_in + 1, 77777, 3, u.data());
            CHECK(ut == 6 && u[2].in_off == 2 * big && u[2].out_off == 2 * 77777 && u[2].tile0 == 4 && u[3].tile0 == 6, "%u -> %u: uniform table", pr.in, pr.out);
        }
    }
    // ---- the pairs that leave the LDS forms, the copy and the refused ones ----
    {
        RsGeom g;
        CHECK(rs_geometry(4001, 4000, g) == MELSPEC_OK && rs_launch(g).mode == kRsLdsSamples && rs_launch(g).lds == rs_span(g.orig, g.width, rs_launch(g).blocks) * 8 && rs_launch(g).lds <= kRsLdsBudget, "4001 -> 4000");
        const RsLaunch l1 = rs_launch(g);
        const RsTable t1 = rs_table(g);
        for (uint64_t len : {uint64_t{1}, uint64_t{4001}, uint64_t{9000}}) check_clip(g, l1, t1, 5, len, 3, false);
        CHECK(rs_geometry(4000, 1, g) == MELSPEC_OK && rs_launch(g).mode == kRsGlobal && rs_launch(g).lds == 0, "4000 -> 1");
        CHECK(rs_geometry(16000, 16000, g) == MELSPEC_OK && g.copy && rs_launch(g).mode == kRsCopy && rs_launch(g).lds == 0, "16000 -> 16000");
        CHECK(rs_geometry(0, 16000, g) == MELSPEC_ERR_INVALID_ARG && rs_geometry(16000, 0, g) == MELSPEC_ERR_INVALID_ARG, "a zero rate");
        CHECK(rs_geometry(4097, 1, g) == MELSPEC_ERR_UNSUPPORTED && rs_geometry(16000, 16001, g) == MELSPEC_ERR_UNSUPPORTED && rs_geometry(2 * 4096, 2, g) == MELSPEC_OK, "the ratio bound");
        // the arguments' helpers
        alignas(16) static char buf[32];
        CHECK(!rs_misaligned(buf + 2, MELSPEC_PCM_S16, buf + 4) && rs_misaligned(buf + 1, MELSPEC_PCM_S16, buf) && rs_misaligned(buf + 2, MELSPEC_PCM_F32, buf) && rs_misaligned(buf, MELSPEC_PCM_F32, buf + 2), "alignment");
        CHECK(rs_dtype_known(0) && rs_dtype_known(1) && !rs_dtype_known(2) && !rs_dtype_known(-1), "dtype codes");
    }
    if (bad) { std::printf("resample_plan_host: %d checks FAILED\n", bad); return 1; }
    std::printf("resample_plan_host: ok\n");
    return 0;
}
