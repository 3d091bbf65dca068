// What the stream banks' planners share (mel_spec_amd/csrc/stream_plan.hpp), on the host: the admission of a push's entries, through
// stream_plan_push and fbank_stream_plan_push, and the key under which the Whisper bank keeps its last plan (PushKey).  HostBank::push is
// the bank's use of the key -- matches once per push; on a miss invalidate, plan, and fill where the frame stage would run -- and every
// expected hit / miss below is written out from the rule, not computed: a push hits iff it repeats the push the key was filled from
// (streams, lengths, pending counts, d_out, offsets present and equal, io code, frames per unit), and a push fills the key iff it emits
// mel rows (no flush) and every stream's idx was >= n_fft before it.
// Links nothing but the headers.  Prints "stream_key_host: ok"; exit status 1 on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "fbank_stream_plan.hpp"
#include "stream_plan.hpp"

using namespace melspec;

static int g_failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                    \
    } while (0)

static const uint32_t kHop = 160;
static float g_rows[2];                                  // stand-ins for two output buffers: only their addresses are used
static const void *const kOut = &g_rows[0], *const kOut2 = &g_rows[1];

struct Push {
    std::vector<uint32_t> ids, lens;
    const void *d_out = kOut;
    std::vector<uint64_t> out_off, src_off;              // empty: absent
    int io = 0, fpu = 6;
    bool flush = false;
};

struct HostBank {
    StreamGeom g = stream_geometry(400, kHop, 80, 3, 4000);
    StreamBook bk;
    PushKey key;
    StreamPlan pl;
    std::string trace;                                   // 'H' / 'M' per push, in order
    HostBank() { bk.reset(3); }
    void push(const Push &p) {
        PushQuery q;
        q.ids = p.ids.data(); q.lens = p.flush ? nullptr : p.lens.data(); q.n = static_cast<uint32_t>(p.ids.size());
        q.fpu = p.fpu; q.io = p.io; q.d_out = p.d_out;
        q.h_out_off = p.out_off.empty() ? nullptr : p.out_off.data();
        q.h_src_off = p.src_off.empty() ? nullptr : p.src_off.data();
        q.repeatable = !p.flush;
        const bool hit = key.matches(bk, q);
        if (!hit) {
            key.invalidate();
            const char *err = nullptr;
            const int rc = stream_plan_push(g, bk, q.ids, q.lens, q.n, p.flush, pl, &err);
            CHECK(rc == 0, "plan refused a push of the sequence: %s", err ? err : "?");
            if (rc) return;
            if (pl.total_frames) key.fill(g, bk, q);     // the frame stage runs when the push emits a row
        }
        stream_commit_push(g, bk, q.ids, q.lens, q.n, p.flush);
        trace += hit ? 'H' : 'M';
    }
    void reset(uint32_t id) { bk.pending[id] = 0; bk.idx[id] = 0; key.invalidate(); }
    // the pushes since the last call
    std::string take() { std::string t; t.swap(trace); return t; }
};

static Push all(std::vector<uint32_t> lens) { Push p; p.ids = {0, 1, 2}; p.lens = std::move(lens); return p; }
static const Push kHops = all({kHop, kHop, kHop});

static void run(HostBank &b, const Push &p, int times, const char *want, const char *what) {
    for (int i = 0; i < times; ++i) b.push(p);
    const std::string got = b.take();
    CHECK(got == want, "%s: got %s, want %s", what, got.c_str(), want);
}

static void test_key() {
    HostBank b;
    // idx before push p is 160 (p - 1): 0, 160, 320 < 400 -- pushes 1-3 cannot fill; push 4 (idx 480) misses and fills; 5-8 repeat it
    run(b, kHops, 8, "MMMMHHHH", "the opening pushes");
    run(b, all({kHop, 2 * kHop, kHop}), 1, "M", "another length");
    run(b, kHops, 5, "MHHHH", "back to one hop");
    Push sub; sub.ids = {0, 2}; sub.lens = {kHop, kHop};
    run(b, sub, 5, "MHHHH", "a subset of the streams");
    run(b, all({37, kHop, kHop}), 1, "M", "a push that leaves a remainder of 37");
    CHECK(b.bk.pending[0] == 37, "pending %u", b.bk.pending[0]);
    run(b, kHops, 4, "MHHH", "the first push after the remainder (pending 37 stays)");
    run(b, all({kHop - 37, kHop, kHop}), 1, "M", "the remainder goes");
    CHECK(b.bk.pending[0] == 0, "pending %u", b.bk.pending[0]);
    run(b, kHops, 6, "MHHHHH", "one hop again");

    Push p = kHops;
    p.d_out = kOut2;
    run(b, p, 2, "MH", "a different d_out");
    run(b, kHops, 2, "MH", "the first d_out again");
    p = kHops; p.out_off = {0, 80, 160};
    run(b, p, 2, "MH", "h_out_off present");
    p.out_off = {0, 160, 320};
    run(b, p, 2, "MH", "h_out_off with other values");
    run(b, kHops, 2, "MH", "h_out_off absent");
    p = kHops; p.io = 1;
    run(b, p, 2, "MH", "a different io code");
    p.io = 1 | 1 << 4;
    run(b, p, 2, "MH", "a different out half of the io code");
    run(b, kHops, 2, "MH", "io 0 again");
    p = kHops; p.src_off = {0, 160, 320};
    run(b, p, 2, "MH", "h_src_off present");
    p.src_off = {0, 200, 400};
    run(b, p, 2, "MH", "h_src_off with other values");
    run(b, kHops, 2, "MH", "h_src_off absent");
    p = kHops; p.fpu = 5;
    run(b, p, 2, "MH", "a changed frames-per-unit");
    run(b, kHops, 2, "MH", "the first frames-per-unit again");

    // a flush never fills: one that emits a row (stream 0 has 37 pending samples), the same one again, then pushes
    run(b, all({37, kHop, kHop}), 1, "M", "a remainder before the flush");
    Push fl; fl.ids = {0, 1, 2}; fl.flush = true;
    run(b, fl, 1, "M", "a flush");
    CHECK(b.pl.total_frames == 1 && !b.key.valid, "the flush emitted %llu rows, key valid %d", static_cast<unsigned long long>(b.pl.total_frames), b.key.valid);
    run(b, fl, 1, "M", "the flush again");
    run(b, kHops, 3, "MHH", "pushes after the flushes");
    {
        PushQuery q;
        q.ids = kHops.ids.data(); q.lens = kHops.lens.data(); q.n = 3; q.fpu = 6; q.d_out = kOut; q.repeatable = false;
        PushKey k;
        CHECK(!k.fill(b.g, b.bk, q) && !k.valid, "fill took a push that cannot come again");
        CHECK(!b.key.matches(b.bk, q), "a push that cannot come again matched");
        q.repeatable = true;
        CHECK(b.key.matches(b.bk, q), "the same push, repeatable, does not match");
    }

    // a reset invalidates: the book of the reset stream looks as it did when the key was filled (pending 0), only the bank knows better
    const PushKey before = b.key;
    b.reset(1);
    {
        PushQuery q;
        q.ids = kHops.ids.data(); q.lens = kHops.lens.data(); q.n = 3; q.fpu = 6; q.d_out = kOut;
        CHECK(before.valid && before.matches(b.bk, q), "the key as it was would have taken the push after the reset");
    }
    // stream 1 starts again: idx 0, 160, 320 before the next three pushes, 480 before the fourth, which fills
    run(b, kHops, 6, "MMMMHH", "pushes after a reset");
}

// the books but for the marks (which a refused push has used)
static bool same_marks_aside(const StreamBook &a, const StreamBook &b) { return a.pending == b.pending && a.idx == b.idx; }
static bool same_marks_aside(const FbankStreamBook &a, const FbankStreamBook &b) { return a.total == b.total && a.emitted == b.emitted && a.pending == b.pending; }

// plan(book, ids, lens, n, &err) -> code; the book has seen a few pushes
template <class Book, class Plan>
static void test_admission(const char *who, Book &bk, Plan plan) {
    struct Case { std::vector<uint32_t> ids, lens; int code; const char *err; };
    const Case cases[] = {
        {{0, 3}, {kHop, kHop}, 1, "stream id out of range"},
        {{0xffffffffu}, {kHop}, 1, "stream id out of range"},
        {{0, 1, 0}, {kHop, kHop, kHop}, 1, "a stream may appear only once per push"},
        {{2, 2}, {0, 0}, 1, "a stream may appear only once per push"},
        {{0, 1}, {kHop, 4001}, 2, "chunk longer than max_chunk"},
        {{1, 1}, {4001, kHop}, 2, "chunk longer than max_chunk"},           // the first problem in entry order is the one reported
    };
    for (const Case &c : cases) {
        const Book before = bk;
        const char *err = nullptr;
        const int rc = plan(bk, c.ids.data(), c.lens.data(), static_cast<uint32_t>(c.ids.size()), &err);
        CHECK(rc == c.code && err && std::strcmp(err, c.err) == 0, "%s: code %d \"%s\", want %d \"%s\"", who, rc, err ? err : "", c.code, c.err);
        CHECK(same_marks_aside(before, bk), "%s: a refused push changed the book", who);
    }
    const uint32_t ids[] = {0, 1, 2}, dup[] = {1, 1}, lens[] = {kHop, 4000, 0};
    const char *err = nullptr;
    CHECK(plan(bk, ids, lens, 3, &err) == 0, "%s: a good push at the limits was refused", who);
    // the epoch wraps: the marks of the pushes before must not read as "seen in this push", and a duplicate is still one
    bk.epoch = 0xffffffffu;
    CHECK(plan(bk, ids, lens, 3, &err) == 0 && bk.epoch == 1, "%s: the push on which the epoch wraps (epoch %u)", who, bk.epoch);
    bk.epoch = 0xffffffffu;
    err = nullptr;
    CHECK(plan(bk, dup, lens, 2, &err) == 1 && err && std::strcmp(err, "a stream may appear only once per push") == 0 && bk.epoch == 1, "%s: a duplicate on the wrapping push", who);
    CHECK(plan(bk, ids, lens, 3, &err) == 0 && bk.epoch == 2, "%s: the push after it", who);
}

int main() {
    test_key();
    {
        const StreamGeom g = stream_geometry(400, kHop, 80, 3, 4000);
        StreamBook bk;
        bk.reset(3);
        const uint32_t ids[] = {0, 1, 2}, lens[] = {500, 37, 0};
        stream_commit_push(g, bk, ids, lens, 3, false);
        StreamPlan pl;
        test_admission("stream_plan_push", bk, [&](StreamBook &b, const uint32_t *i, const uint32_t *l, uint32_t n, const char **err) { return stream_plan_push(g, b, i, l, n, false, pl, err); });
    }
    {
        const FbankStreamGeom g = fbank_stream_geometry(400, kHop, 80, 3, 4000);
        FbankStreamBook bk;
        bk.reset(3);
        const uint32_t ids[] = {0, 1, 2}, lens[] = {500, 37, 0};
        fbank_stream_commit_push(g, bk, ids, lens, 3);
        FbankStreamPlan pl;
        test_admission("fbank_stream_plan_push", bk, [&](FbankStreamBook &b, const uint32_t *i, const uint32_t *l, uint32_t n, const char **err) { return fbank_stream_plan_push(g, b, i, l, n, pl, err); });
    }
    if (g_failures) { std::printf("stream_key_host: %d failures\n", g_failures); return 1; }
    std::printf("stream_key_host: ok\n");
    return 0;
}
