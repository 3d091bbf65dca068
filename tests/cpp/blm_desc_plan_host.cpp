// blm_desc_plan_host.cpp -- the arithmetic of melspec_blm_compute_ragged_device_desc (mel_spec_amd/csrc/blm_desc_plan.hpp): the per-clip
// frame counts the planner kernel shares with the host, the layout of the plan buffer, rules (A) and (B), and the serial planner that
// fills the tables blm_plan_ragged_device_kernel fills.  The yardsticks are restated here, independently: the reference's frame counts
// (src/mel.rs:326-332,387-395: an empty clip has no column; num_frames for center / not; src/mel.rs:751-756: pad_len) and a brute-force
// scan for the prefix, the packed offsets and the block table.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/blm_desc_plan_host.cpp -o /tmp/blm_desc_plan_host && /tmp/blm_desc_plan_host
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "blm_desc_plan.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

static uint64_t lcg_state = 0x9e3779b97f4a7c15ull;
static uint32_t lcg() {
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(lcg_state >> 33);
}

// ---- the reference, restated -----------------------------------------------------------------------------------------------------------
static uint64_t ref_valid(bool center, uint64_t n_fft, uint64_t hop, uint64_t n) {
    if (n == 0) return 0;                                  // samples.is_empty(): cols = 0
    if (center) return n / hop + 1;
    if (n < n_fft) return 0;
    return (n - n_fft) / hop + 1;
}
static uint64_t ref_pad_len(uint64_t len, uint64_t pad_to) {
    if (pad_to == 0) return len;
    uint64_t q = len / pad_to;
    if (len % pad_to) ++q;                                 // div_ceil
    return q * pad_to;
}

struct Want {
    std::vector<uint64_t> off, frames, out_off, prefix, len, valid;
    std::vector<uint32_t> blk;
    uint64_t units = 0;
    uint32_t rejected = 0;
    uint64_t longest = 0;
};
// brute force: the clip of unit u is found by walking the clips, one unit at a time
static Want brute(const BlmDescGeom &g, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, const uint64_t *out_off, uint64_t max_cols,
                  uint64_t max_len) {
    const size_t n = len.size();
    Want w;
    std::vector<uint64_t> eff(n), cols(n);
    uint64_t total = 0;
    for (size_t c = 0; c < n; ++c) {
        const bool rej = len[c] > max_len;
        w.rejected += rej;
        eff[c] = rej ? 0 : len[c];
        cols[c] = ref_pad_len(ref_valid(g.center != 0, g.n_fft, g.hop, eff[c]), g.pad_to);
        total += cols[c];
    }
    if (total > max_cols) {
        w.rejected = static_cast<uint32_t>(n);
        for (size_t c = 0; c < n; ++c) eff[c] = cols[c] = 0;
    }
    uint64_t cursor = 0;
    std::vector<uint32_t> clip_of_unit;
    for (size_t c = 0; c < n; ++c) {
        const uint64_t v = ref_valid(g.center != 0, g.n_fft, g.hop, eff[c]);
        w.off.push_back(off[c]); w.frames.push_back(cols[c]); w.len.push_back(eff[c]); w.valid.push_back(v);
        w.out_off.push_back(out_off ? out_off[c] : cursor * g.n_mels);
        w.prefix.push_back(clip_of_unit.size());
        cursor += cols[c];
        for (uint64_t f = 0; f < cols[c]; f += 4) clip_of_unit.push_back(static_cast<uint32_t>(c));
        w.longest = v > w.longest ? v : w.longest;
    }
    w.units = clip_of_unit.size();
    w.prefix.push_back(w.units);
    for (size_t u = 0; u < clip_of_unit.size(); u += 16) w.blk.push_back(clip_of_unit[u]);
    return w;
}

static void run_case(const BlmDescGeom &g, const std::vector<uint64_t> &off, const std::vector<uint64_t> &len, bool own_offsets, uint64_t max_cols, uint64_t max_len,
                     const char *what) {
    const uint32_t n = static_cast<uint32_t>(len.size());
    std::vector<uint64_t> oo(n);
    for (uint32_t c = 0; c < n; ++c) oo[c] = 1000003ull * (n - c) + 7;
    const Want w = brute(g, off, len, own_offsets ? oo.data() : nullptr, max_cols, max_len);
    const uint64_t max_units = blm_desc_max_units(max_cols, n), max_blocks = blm_desc_max_blocks(max_units);
    const size_t bytes = blm_desc_bytes(n, max_blocks);
    // exactly the bytes the host allocates, filled with a pattern: the sanitizer sees a write past them, the pattern a write that is missing
    std::unique_ptr<uint64_t, decltype(&std::free)> buf(static_cast<uint64_t *>(std::malloc(bytes)), &std::free);
    std::memset(buf.get(), 0xA5, bytes);
    const uint32_t rejected = blm_desc_plan_serial(g, off.data(), len.data(), own_offsets ? oo.data() : nullptr, n, max_cols, max_len, buf.get());
    const BlmDescTables t = blm_desc_tables(buf.get(), n);
    CHECK(rejected == w.rejected, "%s: rejected %u, want %u", what, rejected, w.rejected);
    CHECK(t.prefix[n] == w.units, "%s: units %llu, want %llu", what, (unsigned long long)t.prefix[n], (unsigned long long)w.units);
    CHECK(w.units <= max_units, "%s: %llu units past the bound %llu", what, (unsigned long long)w.units, (unsigned long long)max_units);
    CHECK(w.blk.size() <= max_blocks, "%s: %zu blocks past the table's %llu", what, w.blk.size(), (unsigned long long)max_blocks);
    for (uint32_t c = 0; c < n; ++c) {
        CHECK(t.off[c] == w.off[c] && t.frames[c] == w.frames[c] && t.out_off[c] == w.out_off[c] && t.prefix[c] == w.prefix[c] && t.len[c] == w.len[c] &&
                  t.valid[c] == w.valid[c],
              "%s: clip %u: off %llu/%llu frames %llu/%llu out_off %llu/%llu prefix %llu/%llu len %llu/%llu valid %llu/%llu", what, c, (unsigned long long)t.off[c],
              (unsigned long long)w.off[c], (unsigned long long)t.frames[c], (unsigned long long)w.frames[c], (unsigned long long)t.out_off[c], (unsigned long long)w.out_off[c],
              (unsigned long long)t.prefix[c], (unsigned long long)w.prefix[c], (unsigned long long)t.len[c], (unsigned long long)w.len[c], (unsigned long long)t.valid[c],
              (unsigned long long)w.valid[c]);
        CHECK(t.valid[c] <= t.frames[c] && (g.pad_to == 0 ? t.frames[c] == t.valid[c] : t.frames[c] % g.pad_to == 0 && t.frames[c] - t.valid[c] < g.pad_to), "%s: clip %u", what, c);
    }
    for (size_t k = 0; k < w.blk.size(); ++k) CHECK(t.blk[k] == w.blk[k], "%s: block %zu: clip %u, want %u", what, k, t.blk[k], w.blk[k]);
    CHECK(*t.ctr == 0, "%s: the normaliser's counter", what);
    CHECK(*t.order == blm_desc_norm_order(w.longest), "%s: order %u", what, *t.order);
    // the plan lies inside its buffer, the block table behind the 64-bit words
    CHECK(reinterpret_cast<const char *>(t.blk + max_blocks) <= reinterpret_cast<const char *>(buf.get()) + bytes, "%s: the block table ends past the buffer", what);
    CHECK(reinterpret_cast<const char *>(t.order + 1) <= reinterpret_cast<const char *>(t.blk), "%s: the aux block overlaps the block table", what);
}

int main() {
    const uint64_t edge_len[] = {0, 1, 159, 160, 511, 512, 513, 671, 672};
    const size_t n_edge = sizeof(edge_len) / sizeof(edge_len[0]);

    // ---- per-clip arithmetic against the reference ----
    for (uint32_t center = 0; center < 2; ++center)
        for (uint32_t pad_to : {0u, 1u, 16u}) {
            const BlmDescGeom g{512, 160, pad_to, center, 80};
            std::vector<uint64_t> lens(edge_len, edge_len + n_edge);
            for (int i = 0; i < 3000; ++i) lens.push_back(lcg() % (i % 3 == 0 ? 2000u : 400000u));
            for (uint64_t n : lens) {
                const uint64_t v = ref_valid(center != 0, 512, 160, n), p = ref_pad_len(v, pad_to);
                CHECK(blm_desc_valid_frames(g, n) == v, "valid(%llu) center %u", (unsigned long long)n, center);
                CHECK(blm_desc_padded(g, v) == p, "padded(%llu) pad_to %u", (unsigned long long)v, pad_to);
                const BlmDescClip k = blm_desc_clip(g, n, n);                  // at the bound: accepted
                CHECK(!k.rejected && k.len == n && k.valid == v && k.cols == p && k.units == (p + 3) / 4, "clip(%llu)", (unsigned long long)n);
                if (n > 0) {
                    const BlmDescClip r = blm_desc_clip(g, n, n - 1);          // one past it: a clip of length 0
                    CHECK(r.rejected && r.len == 0 && r.valid == 0 && r.cols == 0 && r.units == 0, "rejected clip(%llu)", (unsigned long long)n);
                }
            }
        }

    // ---- whole plans: clip counts around the planner's 1024 threads, packed and own offsets, the bounds exact / with slack / one short ----
    for (uint32_t n_clips : {1u, 2u, 37u, 1023u, 1024u, 1025u, 2500u})
        for (uint32_t center = 0; center < 2; ++center)
            for (uint32_t pad_to : {0u, 1u, 16u}) {
                const BlmDescGeom g{512, 160, pad_to, center, (n_clips & 1) ? 128u : 80u};
                std::vector<uint64_t> off(n_clips), len(n_clips);
                uint64_t at = 1, longest = 0, total = 0;
                for (uint32_t c = 0; c < n_clips; ++c) {
                    len[c] = lcg() % 3 == 0 ? edge_len[lcg() % n_edge] : lcg() % (c % 97 == 5 ? 200000u : 3000u);
                    off[c] = at;
                    at += len[c] + 1;
                    longest = len[c] > longest ? len[c] : longest;
                    total += ref_pad_len(ref_valid(center != 0, 512, 160, len[c]), pad_to);
                }
                char what[128];
                std::snprintf(what, sizeof(what), "%u clips center %u pad_to %u", n_clips, center, pad_to);
                run_case(g, off, len, false, total, longest, what);                          // exact bounds
                run_case(g, off, len, true, total, longest, what);
                run_case(g, off, len, false, total + 1234, longest * 10 + 1, what);          // slack
                if (total > 0) {
                    run_case(g, off, len, false, total - 1, longest, what);                  // (B): one column short -- all rejected
                    run_case(g, off, len, true, total - 1, longest * 10, what);
                }
                if (longest > 0) {
                    run_case(g, off, len, false, total, longest - 1, what);                  // (A): the longest clip(s) rejected
                    run_case(g, off, len, true, total, longest / 2, what);
                    run_case(g, off, len, false, total, 0, what);                            // every clip with a sample rejected
                    // (A) first, then (B) on what survives: a total that holds exactly the survivors is not (B)
                    uint64_t survivors = 0;
                    for (uint32_t c = 0; c < n_clips; ++c)
                        if (len[c] <= longest / 2) survivors += ref_pad_len(ref_valid(center != 0, 512, 160, len[c]), pad_to);
                    run_case(g, off, len, false, survivors, longest / 2, what);
                    if (survivors > 0) run_case(g, off, len, false, survivors - 1, longest / 2, what);
                }
            }

    // ---- the bounds the host refuses ----
    {
        const BlmDescGeom g{512, 160, 16, 1, 128};
        CHECK(blm_desc_bounds_ok(g, 1, 1), "smallest bounds");
        CHECK(blm_desc_bounds_ok(g, (1ull << 40) - 1, 160ull * ((1ull << 31) - 40)), "largest bounds");
        CHECK(!blm_desc_bounds_ok(g, 1ull << 40, 16000), "2^40 columns");
        CHECK(!blm_desc_bounds_ok(g, 1000, 160ull << 31), "a row of 2^31 columns");
        CHECK(!blm_desc_bounds_ok(g, 1000, ~0ull), "max_clip_samples = 2^64 - 1");
    }

    // ---- the normaliser: the order is 256 / rows-per-workgroup of the host-table call's shape, and a launch sized for a bound has at least
    // as many threads per row as the order of EVERY shorter clip (the order cannot be followed otherwise) ----
    {
        uint32_t most = 0;
        bool past_lds = false;
        for (uint64_t longest = 0; longest < 60000; ++longest) {
            const uint32_t o = blm_desc_norm_order(longest);
            size_t stride, per, lstride, lper;
            int per_cu, lper_cu;
            blm_norm_shape_ragged(longest, stride, per, per_cu);
            CHECK(o == (per ? 256 / per : 0), "order(%llu)", (unsigned long long)longest);
            CHECK(o != 0 || longest > 30000, "order(%llu) = 0", (unsigned long long)longest);
            if (o == 0) { past_lds = true; continue; }
            CHECK(!past_lds, "order(%llu) = %u behind a length that did not fit LDS", (unsigned long long)longest, o);
            most = o > most ? o : most;
            blm_desc_norm_launch(longest, lstride, lper, lper_cu);
            CHECK(lper >= 1 && lper <= per && lstride == stride, "launch(%llu): %zu rows of %zu floats", (unsigned long long)longest, lper, lstride);
            CHECK(256 / lper >= most, "launch(%llu) has %zu threads per row, a shorter clip's order is %u", (unsigned long long)longest, 256 / lper, most);
            CHECK((lper * lstride + 2 * lper + 256 + 4 * lper + 4) * sizeof(float) <= (lper_cu == 1 ? 160u : 40u) * 1024, "launch(%llu): LDS", (unsigned long long)longest);
        }
        CHECK(past_lds, "no length up to 60000 frames left LDS");
        CHECK(blm_desc_norm_order(1ull << 31) == 0, "2^31 valid frames");
    }

    if (bad) {
        std::printf("blm_desc_plan_host: %d checks failed\n", bad);
        return 1;
    }
    std::printf("blm_desc_plan_host: ok\n");
    return 0;
}
