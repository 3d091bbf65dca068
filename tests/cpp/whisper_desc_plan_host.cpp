// whisper_desc_plan_host.cpp -- the plan of the centred Whisper features on a clip table in device memory
// (melspec_whisper_compute_ragged_device_desc*; mel_spec_amd/csrc/whisper_centered_plan.hpp: wc_desc_*).  The per-thread functions of
// wc_plan_desc_kernel are run here serially for 1024 "threads" -- count, an exclusive sum of the counts, write -- and every table entry
// is compared with what wc_plan builds on the host for the same tables: the records, the interior (offset, the length whose un-centred
// frame count is the interior, the row offset), the compacted edge list in clip order, the edge launch's batch, the true counts and the
// block table within its capacity; then the argument verdicts in their order.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/whisper_desc_plan_host.cpp -o /tmp/wd && /tmp/wd
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "whisper_centered_plan.hpp"

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

// plan_ragged_device_kernel's frame count of a clip of n samples (frame_len 400, frame_shift 160)
static uint64_t frames(uint64_t n) { return n < 400 ? 0 : (n - 400) / 160 + 1; }

static long checked = 0;

// one batch: the planner's three steps for 1024 threads against wc_plan
static void run(const std::vector<uint64_t> &len, uint64_t pad_to, int n_mels, bool split, bool own_offsets, const char *what) {
    const uint32_t n = static_cast<uint32_t>(len.size());
    std::vector<uint64_t> off(n), dst(n);
    uint64_t cur = 1;
    for (uint32_t i = 0; i < n; ++i) { off[i] = cur; cur += len[i] + 1 + lcg() % 3; }
    const uint64_t T = pad_to / 160;
    cur = 0;
    for (uint32_t k = 0; k < n; ++k) {          // reverse clip order with gaps
        const uint32_t i = n - 1 - k;
        cur += 1 + lcg() % 7;
        dst[i] = cur;
        cur += T * n_mels;
    }
    const uint64_t *d = own_offsets ? dst.data() : nullptr;
    // wc_plan lists a clip's edge frames through the helpers the planner uses (wc_edge_count / wc_edge_frame), so the edge lists below
    // compare the compaction, the offsets and the order, not the enumeration: that is checked on its own, frame by frame against wc_class,
    // at the top of main() (and by tests/cpp/whisper_centered_host.cpp), which is what gives this comparison its meaning
    const WcBatch want = wc_plan(off.data(), len.data(), 0, n, pad_to, n_mels, split ? d : nullptr, split ? nullptr : d);

    const size_t bytes = wc_desc_bytes(n);
    CHECK(bytes % 16 == 0, "%s: %zu bytes", what, bytes);
    // exactly the buffer's size, every byte a pattern: ASan sees a write past it, the comparison an entry that was not written
    std::vector<unsigned char> raw(bytes ? bytes : 1, 0xA5);
    unsigned char *buf = static_cast<unsigned char *>(std::malloc(bytes ? bytes : 1));
    std::memcpy(buf, raw.data(), bytes);
    const WcDescTables t = wc_desc_tables(buf, n);
    CHECK(reinterpret_cast<unsigned char *>(t.e_map + wc_desc_cap(n)) <= buf + bytes, "%s: the tables end past wc_desc_bytes", what);
    WcDescIn q{};
    q.off = off.data(); q.len = len.data(); q.rows_off = split ? d : nullptr; q.out_off = split ? nullptr : d;
    q.n_clips = n; q.n_mels = static_cast<uint32_t>(n_mels); q.pad_to = pad_to;

    std::vector<uint64_t> part(kWcDescThreads);
    uint32_t covered = 0;
    for (uint32_t tid = 0; tid < kWcDescThreads; ++tid) {
        uint32_t c0, c1;
        wc_desc_slice(n, tid, c0, c1);
        CHECK(c0 == covered && c1 >= c0 && c1 <= n, "%s: thread %u owns [%u, %u) after %u", what, tid, c0, c1, covered);
        covered = c1;
        part[tid] = wc_desc_count(q, c0, c1);
    }
    CHECK(covered == n, "%s: the slices cover %u of %u clips", what, covered, n);
    uint64_t total = 0;
    for (uint32_t tid = 0; tid < kWcDescThreads; ++tid) { const uint64_t p = part[tid]; part[tid] = total; total += p; }
    *t.n_edges = total;
    for (uint32_t tid = 0; tid < kWcDescThreads; ++tid) {
        uint32_t c0, c1;
        wc_desc_slice(n, tid, c0, c1);
        wc_desc_fixed(t, n, tid);
        wc_desc_write(q, t, c0, c1, part[tid]);
    }

    const uint64_t cap = wc_desc_cap(n);
    CHECK(total == want.edges.size() && total <= cap, "%s: %llu edges, wc_plan has %zu, capacity %llu", what, (unsigned long long)total, want.edges.size(), (unsigned long long)cap);
    uint64_t interior = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const WcRecord &r = t.rec[i], &w = want.records[i];
        CHECK(r.rows_off == w.rows_off && r.out_off == w.out_off && r.T == w.T && r.first_silent == w.first_silent, "%s: record %u", what, i);
        CHECK(r.T == T, "%s: clip %u has %llu frames", what, i, (unsigned long long)r.T);
        CHECK(t.in_off[i] == want.in_off[i] && t.in_out_off[i] == want.in_out_off[i], "%s: interior of clip %u", what, i);
        CHECK(frames(t.in_len[i]) == want.in_frames[i], "%s: clip %u: length %llu gives %llu frames, the interior has %llu", what, i, (unsigned long long)t.in_len[i],
              (unsigned long long)frames(t.in_len[i]), (unsigned long long)want.in_frames[i]);
        // the interior's last frame ends inside the samples the call may read
        CHECK(t.in_len[i] == 0 || 120 + t.in_len[i] <= want.clips[i].n_eff, "%s: clip %u: the interior reads past n_eff", what, i);
        interior += want.in_frames[i];
        ++checked;
    }
    CHECK(interior == want.interior_frames && interior <= wc_desc_interior_bound(n, pad_to), "%s: %llu interior frames, bound %llu", what, (unsigned long long)interior,
          (unsigned long long)wc_desc_interior_bound(n, pad_to));
    for (uint64_t e = 0; e < total && e < want.edges.size(); ++e) {
        const WcEdge &g = t.edges[e], &w = want.edges[e];
        CHECK(g.pcm_off == w.pcm_off && g.n_eff == w.n_eff && g.P == w.P && g.t == w.t && g.row_off == w.row_off && g.clip == w.clip, "%s: edge %llu", what, (unsigned long long)e);
        CHECK(t.e_out_off[e] == w.row_off && t.e_map[e] == w.clip, "%s: edge %llu of the launch's batch", what, (unsigned long long)e);
        // no unit stores outside its clip's rows
        const WcRecord &r = want.records[w.clip];
        CHECK(t.e_out_off[e] >= r.rows_off && t.e_out_off[e] + n_mels <= r.rows_off + r.T * n_mels, "%s: edge %llu stores outside its clip", what, (unsigned long long)e);
        ++checked;
    }
    for (uint64_t e = 0; e < cap; ++e)
        CHECK(t.e_off[e] == 400 * e && t.e_frames[e] == 1 && t.e_prefix[e] == e, "%s: slot %llu of the edge batch", what, (unsigned long long)e);
    for (uint64_t e = cap; e < cap + 5; ++e) CHECK(t.e_prefix[e] == cap, "%s: prefix past the capacity", what);
    // the block table: the "clip" (edge) that holds unit 16 k, for every block below its capacity
    for (uint64_t b = 0; b < wc_desc_blocks(n); ++b) CHECK(t.e_blk[b] == 16 * b && (16 * b < cap || b == cap / 16), "%s: block %llu", what, (unsigned long long)b);
    std::free(buf);
}

static std::vector<uint64_t> random_lengths(uint32_t n, uint64_t top) {
    std::vector<uint64_t> v(n);
    for (auto &x : v) x = lcg() % (top + 1);
    return v;
}

static void verdicts() {
    int x = 0;
    const void *p = &x, *odd = reinterpret_cast<const char *>(&x) + 1;
    const int F32 = MELSPEC_PCM_F32, S16 = MELSPEC_PCM_S16, O32 = MELSPEC_OUT_F32, O16 = MELSPEC_OUT_F16;
    auto is = [](const WcArgs &a, WcVerdict v, int status, const char *word) {
        return a.verdict == v && a.status == status && (word == nullptr ? true : (a.msg != nullptr && std::strstr(a.msg, word) != nullptr));
    };
    // each line fails for the reason named and for every later reason too: the earlier one wins
    CHECK(is(wc_args_desc_io(false, false, true, 9, 9, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "NULL"), "1 ctx");
    CHECK(is(wc_args_desc_io(true, false, true, 9, O32, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "pcm_dtype"), "2 pcm code");
    CHECK(is(wc_args_desc_io(true, false, true, S16, 9, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "out_dtype"), "2 out code");
    CHECK(is(wc_args_desc_io(true, false, false, 9, 9, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_UNSUPPORTED, nullptr), "the f32 calls have no codes");
    CHECK(is(wc_args_desc_io(true, false, true, S16, O16, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_UNSUPPORTED, nullptr), "3 support");
    CHECK(wc_args_desc_io(true, false, true, S16, O16, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr).msg == nullptr, "3: the caller names the geometry");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 0, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "fixed width"), "4 pad_to 0");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 399, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "at least 400"), "4 pad_to 399");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, 0, nullptr, nullptr, nullptr, nullptr, true, nullptr), kWcDone, MELSPEC_OK, nullptr), "5 no clips");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, 1, nullptr, p, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "offset/length"), "6 offsets");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, 1, p, nullptr, nullptr, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "offset/length"), "6 lengths");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, 1, p, p, nullptr, odd, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"), "7 pcm");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, 1, p, p, odd, nullptr, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"), "7 destination");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, 1, p, p, odd, odd, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "d_clip_max"), "8 clip_max");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, kWcDescMaxClips + 1, p, p, odd, p, true, p), kWcFail, MELSPEC_ERR_INVALID_ARG, "aligned"), "9 pcm alignment");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, kWcDescMaxClips + 1, p, p, p, odd, false, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "aligned"), "9 out alignment");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, kWcDescMaxClips + 1, p, p, p, p, true, p), kWcFail, MELSPEC_ERR_INVALID_ARG, "too many"), "10 clips");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O16, 400, kWcDescMaxClips, p, p, p, p, true, p), kWcGo, MELSPEC_OK, nullptr), "go");
    CHECK(is(wc_args_desc_io(true, true, true, F32, O32, 400, 1, p, p, odd, odd, false, nullptr), kWcGo, MELSPEC_OK, nullptr), "(F32, F32) is the f32 call: no alignment verdict");
    CHECK(is(wc_args_desc_io(true, true, true, S16, O32, 400, 1, p, p, reinterpret_cast<const char *>(&x) + 2, p, false, nullptr), kWcGo, MELSPEC_OK, nullptr), "an int16 clip at an odd sample");
    // the f32 calls
    CHECK(is(wc_args_desc(false, true, 400, 1, p, p, p, p, false, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "NULL"), "f32: ctx");
    CHECK(is(wc_args_desc(true, true, 0, 1, p, p, p, p, false, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "fixed width"), "f32: pad_to");
    CHECK(is(wc_args_desc(true, true, 480000, 3, p, p, p, p, true, nullptr), kWcFail, MELSPEC_ERR_INVALID_ARG, "d_clip_max"), "f32: clip_max");
    CHECK(is(wc_args_desc(true, true, 480000, 3, p, p, p, p, false, nullptr), kWcGo, MELSPEC_OK, nullptr), "f32: go");
    CHECK(kWcDescMaxClips == 0xffffffffu / 5, "the clip bound");
}

int main() {
    // the edge helpers against the definition of the classes, frame by frame
    for (uint64_t pad_to : {400ull, 401ull, 559ull, 560ull, 1600ull, 4799ull, 4800ull, 4801ull, 4959ull, 10240ull, 10880ull, 20480ull, 480000ull}) {
        std::vector<uint64_t> ns = {0, 1, 199, 200, 201, 399, 400, 560, 2400, 1000, 10040, 10239, 20000, 9000};
        for (uint64_t k = 0; k <= 202; ++k)
            if (pad_to + 1 >= k) ns.push_back(pad_to + 1 - k);
        for (uint64_t n : ns) {
            const WcClip c = wc_clip(n, pad_to);
            uint64_t te[kWcMaxEdges], k = 0;
            const unsigned ne = wc_edges(c, te);
            CHECK(ne == wc_edge_count(c) && ne <= kWcMaxEdges, "pad_to %llu n %llu: %u edges", (unsigned long long)pad_to, (unsigned long long)n, ne);
            for (uint64_t t = 0; t < c.T; ++t)
                if (wc_class(c, t) == kWcEdge) { CHECK(k < ne && te[k] == t && wc_edge_frame(c, (unsigned)k) == t, "pad_to %llu n %llu: edge %llu", (unsigned long long)pad_to, (unsigned long long)n, (unsigned long long)k); ++k; }
            CHECK(k == ne, "pad_to %llu n %llu: %llu edge frames by class, %u listed", (unsigned long long)pad_to, (unsigned long long)n, (unsigned long long)k, ne);
        }
    }
    const std::vector<uint64_t> padded = {0, 1, 199, 200, 201, 399, 400, 2400, 4599, 4600, 4601, 4799, 4800, 9000};
    const std::vector<uint64_t> tiles = {0, 1000, 10040, 10239, 20000};
    for (int nm : {80, 128})
        for (int split = 0; split < 2; ++split)
            for (int own = 0; own < 2; ++own) {
                run(padded, 4800, nm, split, own, "test 1");
                for (uint64_t pad_to : {400ull, 401ull, 559ull, 560ull, 4799ull, 4801ull, 4959ull}) {
                    std::vector<uint64_t> ns = {0, 1, 200, 399, 400, 560, pad_to - 201, pad_to - 200, pad_to - 1, pad_to, pad_to + 1, pad_to + 500};
                    run(ns, pad_to, nm, split, own, "test 2");
                }
                for (uint64_t pad_to : {10240ull, 10880ull, 20480ull}) run(tiles, pad_to, nm, split, own, "test 3");
                for (uint64_t pad_to : {1600ull, 4800ull, 10240ull, 480000ull}) {
                    std::vector<uint64_t> ns;
                    for (uint64_t k = 0; k <= 202; ++k) ns.push_back(pad_to + 1 - k);
                    run(ns, pad_to, nm, split, own, "around pad_to");
                }
            }
    for (uint32_t n : {0u, 1u, 5u, 1023u, 1024u, 1025u, 2500u})
        for (int own = 0; own < 2; ++own) {
            run(random_lengths(n, 2000), 1600, 80, own != 0, own != 0, "test 4");
            run(random_lengths(n, 500000), 480000, 128, false, own != 0, "30 s");
        }
    verdicts();
    if (bad) { std::printf("whisper_desc_plan_host: %d checks FAILED\n", bad); return 1; }
    std::printf("whisper_desc_plan_host: ok (%ld clips and edges compared)\n", checked);
    return 0;
}
