// The NeMo / Parakeet stream bank's bookkeeping (mel_spec_amd/csrc/blm_stream_plan.hpp) on the host: the bank's slots are a float array,
// scatter and carry are the loops of the kernels in aux_kernels.hpp, and the frame kernel's place is taken by its rule for a tap: frame f
// of a clip (off, len, org0) reads clip index org0 + f * hop + t for t in [0, 400); an index outside [0, len) is a zero; index 0 has no
// predecessor (it is not pre-emphasised); every other index is pre-emphasised with the sample in front of it.  Every emitted frame's taps,
// read that way from the state, must be the taps of the same frame of the whole clip -- value, predecessor and "is padding" alike --
// where "no predecessor" may only ever mean the stream's sample 0.
// Stand-alone: no library.  Prints "blm_stream_host: ok" and the first-push counts; exit status 1 on any mismatch.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "blm_stream_plan.hpp"

using namespace melspec;

static int g_failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                    \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() { g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull; return static_cast<uint32_t>(g_rng >> 33); }
static float noise() { return (static_cast<float>(rnd() & 0xffff) - 32768.0f) * (0.4f / 32768.0f) + 1.0f; }     // never 0, never the stale value

constexpr float kStale = 1.0e6f;         // what a slot held before: a tap that reads in front of or behind its stream's samples shows

struct Tap {
    bool pad, has_prev;
    float cur, prev;
    bool operator==(const Tap &o) const {
        return pad == o.pad && (pad || (cur == o.cur && has_prev == o.has_prev && (!has_prev || prev == o.prev)));
    }
};
// the kernel's rule on a clip
static Tap clip_tap(const float *clip, int64_t len, int64_t idx) {
    if (idx < 0 || idx >= len) return Tap{true, false, 0.0f, 0.0f};
    return Tap{false, idx != 0, clip[idx], idx != 0 ? clip[idx - 1] : 0.0f};
}

// src/mel.rs num_frames
static uint64_t ref_frames(bool center, uint32_t hop, uint64_t n) {
    if (center) return n == 0 ? 0 : n / hop + 1;
    return n < 512 ? 0 : (n - 512) / hop + 1;
}

struct HostBank {
    BlmStreamGeom g;
    BlmStreamBook bk;
    std::vector<float> state;
    uint32_t max_keep = 0;
    HostBank(uint32_t hop, bool center, uint32_t n_streams, uint32_t max_chunk) {
        g = blm_stream_geometry(hop, center, 80, n_streams, max_chunk);
        bk.reset(n_streams);
        state.assign(static_cast<size_t>(n_streams) * g.stride, kStale);
    }
    // 0 or the plan's error code.  x[s]: everything stream s has received once this call is through; the frames' taps are checked here.
    int push(const std::vector<uint32_t> &ids, const std::vector<std::vector<float>> &chunks, bool finish, const std::vector<std::vector<float>> &x, BlmStreamPlan &pl) {
        std::vector<uint32_t> lens;
        for (const auto &c : chunks) lens.push_back(static_cast<uint32_t>(c.size()));
        const char *err = "";
        const uint32_t n = static_cast<uint32_t>(ids.size());
        if (const int rc = blm_stream_plan_push(g, bk, ids.data(), finish ? nullptr : lens.data(), n, finish, pl, &err)) return rc;
        for (uint32_t i = 0; i < n && !finish; ++i) {     // scatter
            const StreamEntry &e = pl.entries[i];
            CHECK(e.len == lens[i] && e.stream == ids[i], "entry %u", i);
            if (e.len) std::memcpy(&state[e.stream * g.stride + g.in_off], chunks[i].data(), e.len * sizeof(float));
        }
        uint64_t cursor = 0;
        for (uint32_t i = 0; i < n; ++i) {                // frames
            const uint32_t s = ids[i];
            CHECK(pl.out_off[i] == cursor && pl.entries[i].out_off == cursor && pl.entries[i].frames == pl.frames[i], "rows of entry %u are not packed", i);
            cursor += pl.frames[i] * g.n_mels;
            if (!pl.frames[i]) continue;
            const std::vector<float> &whole = x[s];
            const int64_t total = static_cast<int64_t>(whole.size());
            CHECK(pl.off[i] >= static_cast<uint64_t>(s) * g.stride && pl.off[i] + pl.len[i] <= static_cast<uint64_t>(s + 1) * g.stride, "clip of entry %u leaves its slot", i);
            const float *clip = &state[pl.off[i]];
            for (uint64_t f = 0; f < pl.frames[i]; ++f) {
                const int64_t k = static_cast<int64_t>(bk.emitted[s] + f);
                const int64_t org = pl.org0[i] + static_cast<int64_t>(f) * g.hop, gorg = k * g.hop + g.org0;
                if (!finish) CHECK(gorg + 400 <= total, "stream %u frame %" PRId64 " emitted before its samples were there", s, k);
                for (int t = 0; t < 400; ++t) {
                    const Tap a = clip_tap(clip, static_cast<int64_t>(pl.len[i]), org + t), b = clip_tap(whole.data(), total, gorg + t);
                    if (!(a == b)) { CHECK(false, "stream %u frame %" PRId64 " tap %d: (%d %g %d %g) != (%d %g %d %g)", s, k, t, a.pad, a.cur, a.has_prev, a.prev, b.pad, b.cur, b.has_prev, b.prev); break; }
                }
            }
        }
        for (uint32_t i = 0; i < n; ++i) {                // carry
            const StreamEntry &e = pl.entries[i];
            CHECK(e.keep <= g.in_off && e.keep < (g.center ? 401u : 457u), "carry of %u samples (in_off %u)", e.keep, g.in_off);
            if (e.keep > max_keep) max_keep = e.keep;
            if (!e.len) continue;
            float *slot = &state[e.stream * g.stride];
            std::memmove(slot + g.in_off - e.keep, slot + g.in_off + e.len - e.keep, e.keep * sizeof(float));
        }
        blm_stream_commit_push(g, bk, ids.data(), finish ? nullptr : lens.data(), n, finish);
        return 0;
    }
};

static bool same_book(const BlmStreamBook &a, const BlmStreamBook &b) { return a.total == b.total && a.emitted == b.emitted && a.ended == b.ended; }

static void drive(uint32_t hop, bool center, uint32_t max_chunk) {
    const uint32_t n_streams = 5;
    const uint32_t target = hop == 1 ? 1500 : 7000;
    HostBank b(hop, center, n_streams, max_chunk);
    CHECK(b.g.hop == hop && b.g.in_off % 4 == 0 && b.g.in_off >= (center ? 401u : 457u) && b.g.org0 == (center ? -200 : 56), "geometry of hop %u", hop);
    std::vector<std::vector<float>> src(n_streams), fed(n_streams);
    std::vector<uint64_t> emitted(n_streams, 0);
    // stream 4 stays short (a finish soon after the start), stream 3 empty
    const uint32_t targets[5] = {target, target - 37, target / 2 + 1, 0, 150};
    for (uint32_t s = 0; s < n_streams; ++s) { src[s].resize(targets[s]); for (auto &v : src[s]) v = noise(); }
    std::vector<uint32_t> pos(n_streams, 0);
    const uint32_t sizes[12] = {0, 1, hop - 1, hop, hop + 1, 199, 200, 201, 399, 400, 401, max_chunk};
    uint32_t live = 0;
    for (uint32_t s = 0; s < n_streams; ++s) live += targets[s] > 0;
    while (live) {
        std::vector<uint32_t> ids;
        std::vector<std::vector<float>> chunks;
        for (uint32_t s = 0; s < n_streams; ++s) {
            if (pos[s] >= targets[s] || rnd() % 10 >= 7) continue;
            uint32_t len = sizes[rnd() % 12];
            if (len > max_chunk) len = max_chunk;
            if (len > targets[s] - pos[s]) len = targets[s] - pos[s];
            ids.push_back(s);
            chunks.emplace_back(src[s].begin() + pos[s], src[s].begin() + pos[s] + len);
        }
        if (ids.empty()) continue;
        std::vector<size_t> want;
        for (size_t i = 0; i < ids.size(); ++i) {
            want.push_back(blm_stream_frames_after(b.g, b.bk, ids[i], static_cast<uint32_t>(chunks[i].size())));
            fed[ids[i]].insert(fed[ids[i]].end(), chunks[i].begin(), chunks[i].end());
        }
        BlmStreamPlan pl;
        const int rc = b.push(ids, chunks, false, fed, pl);
        CHECK(rc == 0, "push refused: %d", rc);
        for (size_t i = 0; i < ids.size(); ++i) {
            CHECK(pl.frames[i] == want[i], "frames_after said %zu, the push emitted %" PRIu64, want[i], pl.frames[i]);
            emitted[ids[i]] += pl.frames[i];
            pos[ids[i]] += static_cast<uint32_t>(chunks[i].size());
            if (pos[ids[i]] >= targets[ids[i]]) --live;
        }
    }
    // finish: a random order, two calls
    for (int part = 0; part < 2; ++part) {
        std::vector<uint32_t> ids = part ? std::vector<uint32_t>{3, 0, 4} : std::vector<uint32_t>{2, 1};
        std::vector<size_t> want;
        for (uint32_t s : ids) want.push_back(blm_stream_finish_frames(b.g, b.bk, s));
        BlmStreamPlan pl;
        const int rc = b.push(ids, std::vector<std::vector<float>>(ids.size()), true, fed, pl);
        CHECK(rc == 0, "finish refused: %d", rc);
        for (size_t i = 0; i < ids.size(); ++i) {
            CHECK(pl.frames[i] == want[i], "finish_frames said %zu, the finish emitted %" PRIu64, want[i], pl.frames[i]);
            if (!center) CHECK(pl.frames[i] == 0, "a finish without centre padding emitted %" PRIu64 " frames", pl.frames[i]);
            if (center && hop >= 120) CHECK(pl.frames[i] <= 2, "a finish emitted %" PRIu64 " frames at hop %u", pl.frames[i], hop);
            emitted[ids[i]] += pl.frames[i];
        }
    }
    for (uint32_t s = 0; s < n_streams; ++s) {
        CHECK(fed[s] == src[s], "stream %u: fed %zu of %zu samples", s, fed[s].size(), src[s].size());
        CHECK(emitted[s] == ref_frames(center, hop, src[s].size()) && b.bk.emitted[s] == emitted[s], "stream %u (%zu samples, hop %u, center %d): %" PRIu64 " frames, num_frames says %" PRIu64, s,
              src[s].size(), hop, center, emitted[s], ref_frames(center, hop, src[s].size()));
        CHECK(b.bk.ended[s] == 1 && blm_stream_frames_after(b.g, b.bk, s, 400) == 0 && blm_stream_finish_frames(b.g, b.bk, s) == 0, "stream %u is not ended", s);
    }
    // an ended stream refuses a push and a second finish; a refused call changes nothing (the marks aside)
    {
        const BlmStreamBook before = b.bk;
        const std::vector<float> st = b.state;
        BlmStreamPlan pl;
        CHECK(b.push({0}, {std::vector<float>(10, 0.5f)}, false, fed, pl) == 1, "a push to an ended stream was admitted");
        CHECK(b.push({1}, {std::vector<float>()}, true, fed, pl) == 1, "a second finish was admitted");
        CHECK(same_book(before, b.bk) && st == b.state, "a refused call changed the bank");
        b.bk.reset_one(0);
        CHECK(blm_stream_frames_after(b.g, b.bk, 0, 512) == (center ? (512 - 200) / hop + 1 : 1), "a reset stream does not start afresh");
    }
    std::printf("hop %u center %d max_chunk %u: longest carry %u of %u\n", hop, center, max_chunk, b.max_keep, b.g.in_off);
}

int main() {
    const uint32_t hops[4] = {160, 120, 400, 1}, chunks[3] = {160, 517, 2000};
    for (uint32_t hop : hops)
        for (int center = 0; center < 2; ++center)
            for (uint32_t mc : chunks) drive(hop, center != 0, mc);
    // the plan's refusals, each leaving the book as it was
    {
        HostBank b(160, true, 3, 1000);
        std::vector<std::vector<float>> fed(3);
        BlmStreamPlan pl;
        fed[0].assign(500, 1.5f);
        CHECK(b.push({0}, {fed[0]}, false, fed, pl) == 0 && pl.frames[0] == 2, "500 samples: %" PRIu64 " frames", pl.frames[0]);
        const BlmStreamBook before = b.bk;
        const std::vector<float> st = b.state;
        const std::vector<float> ten(10, 0.5f), big(1001, 0.5f);
        CHECK(b.push({3}, {ten}, false, fed, pl) == 1, "id out of range");
        CHECK(b.push({1, 1}, {ten, ten}, false, fed, pl) == 1, "an id twice");
        CHECK(b.push({1, 0}, {ten, big}, false, fed, pl) == 2, "a chunk over max_chunk");
        CHECK(b.push({0, 0}, {ten, ten}, true, fed, pl) == 1, "an id twice in a finish");
        CHECK(same_book(before, b.bk) && st == b.state, "a refused push changed the bank");
    }
    // the first pushes of one hop each, centred: frame k is there with k * 160 + 200 samples
    {
        HostBank b(160, true, 1, 160);
        std::vector<std::vector<float>> fed(1);
        std::printf("first_pushes");
        for (int k = 0; k < 5; ++k) {
            std::vector<float> c(160);
            for (auto &v : c) v = noise();
            fed[0].insert(fed[0].end(), c.begin(), c.end());
            BlmStreamPlan pl;
            CHECK(b.push({0}, {c}, false, fed, pl) == 0, "push %d", k);
            std::printf(" %" PRIu64, pl.frames[0]);
        }
        std::printf(" finish %zu\n", blm_stream_finish_frames(b.g, b.bk, 0));
    }
    if (g_failures) { std::printf("blm_stream_host: %d failures\n", g_failures); return 1; }
    std::printf("blm_stream_host: ok\n");
    return 0;
}
