// whisper_centered_host.cpp -- the host side of the centred Whisper features (melspec_whisper_*) that is arithmetic only
// (mel_spec_amd/csrc/whisper_centered_plan.hpp): the frame count and the class of every frame against literal tables, every frame in
// exactly one class, the gather rule against a reflect-padded signal built here, the interior table's offsets and output offsets, the
// edge list, and the order of the argument verdicts.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/whisper_centered_host.cpp -o /tmp/whisper_centered_host && /tmp/whisper_centered_host
#include <cstdio>
#include <cstring>
#include <string>
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

// the classes of a clip's frames as a string: E edge, I interior, S silent
static std::string classes(uint64_t n, uint64_t pad_to) {
    const WcClip c = wc_clip(n, pad_to);
    std::string s;
    for (uint64_t t = 0; t < c.T; ++t) s += "IES"[wc_class(c, t)];
    return s;
}
static std::string rep(const char *a, int na, const char *b = "", int nb = 0, const char *c = "", int nc = 0) {
    std::string s;
    for (int i = 0; i < na; ++i) s += a;
    for (int i = 0; i < nb; ++i) s += b;
    for (int i = 0; i < nc; ++i) s += c;
    return s;
}

int main() {
    // ---- literal tables: T and the class of every frame ----
    // pad_to = 0: no silent frame; frames 0, 1 mirror at 0; the interior starts at t = 2 once n >= 520; the tail is edge
    const struct { uint64_t n; const char *want; } plain[] = {
        {399, ""},       {400, "EE"},      {401, "EE"},      {559, "EEI"},     {560, "EEI"},     {599, "EEI"},   {600, "EEI"},
        {639, "EEI"},    {640, "EEIE"},    {679, "EEIE"},    {680, "EEII"},    {1119, "EEIIII"}, {1120, "EEIIIIE"}};
    for (const auto &p : plain) {
        const std::string got = classes(p.n, 0);
        CHECK(got == p.want, "pad_to 0, n %llu: %s, want %s", (unsigned long long)p.n, got.c_str(), p.want);
        CHECK(wc_num_frames(p.n, 0) == std::strlen(p.want), "pad_to 0, n %llu: T", (unsigned long long)p.n);
    }
    // (frame 2 reads s[120 .. 520): interior from n = 520; n = 480 .. 519 has a third frame that mirrors at P - 1)
    CHECK(classes(519, 0) == "EEE" && classes(520, 0) == "EEI" && classes(479, 0) == "EE", "the first interior frame");
    // pad_to = 4800: T = 30 whatever n
    const struct { uint64_t n; std::string want; } padded[] = {
        {0, rep("S", 30)},
        {1, rep("E", 2, "S", 28)},                       // 160 * 2 - 200 = 120 >= 1: frame 2 onwards reads zeros only
        {199, rep("E", 3, "S", 27)},                     // frame 2 starts at 120 < 199; frame 3 at 280
        {200, rep("E", 3, "S", 27)},
        {201, rep("E", 3, "S", 27)},
        {399, rep("E", 4, "S", 26)},                     // frame 3 starts at 280 < 399; frame 4 at 440
        {400, rep("E", 4, "S", 26)},
        {4599, rep("E", 2, "I", 26, "E", 2)},            // 160 * 27 + 200 = 4520 <= 4599 < 4680: frames 2 .. 27; frames 28, 29 straddle
        {4600, rep("E", 2, "I", 26, "E", 2)},
        {4601, rep("E", 2, "I", 26, "E", 2)},
        {4799, rep("E", 2, "I", 27, "E", 1)},            // 160 * 28 + 200 = 4680 <= 4799: frames 2 .. 28; frame 29 mirrors at P - 1
        {4800, rep("E", 2, "I", 27, "E", 1)},
        {4801, rep("E", 2, "I", 27, "E", 1)},            // trimmed to 4800
        {9000, rep("E", 2, "I", 27, "E", 1)}};
    for (const auto &p : padded) {
        const std::string got = classes(p.n, 4800);
        CHECK(got == p.want, "pad_to 4800, n %llu: %s, want %s", (unsigned long long)p.n, got.c_str(), p.want.c_str());
        CHECK(wc_num_frames(p.n, 4800) == 30, "pad_to 4800, n %llu: T", (unsigned long long)p.n);
    }
    CHECK(wc_num_frames(0, 0) == 0 && wc_num_frames(479999, 480000) == 3000 && wc_num_frames(176000, 0) == 1100, "frame counts");

    // ---- every frame once; the classes against the definition, sample by sample ----
    for (uint64_t pad_to : {uint64_t(0), uint64_t(400), uint64_t(401), uint64_t(4800), uint64_t(4801), uint64_t(4959)}) {
        for (uint64_t n = 0; n <= 5400; ++n) {
            const WcClip c = wc_clip(n, pad_to);
            uint64_t count[3] = {0, 0, 0};
            for (uint64_t t = 0; t < c.T; ++t) {
                const WcClass k = wc_class(c, t);
                ++count[k];
                bool any = false, mirrored = false, beyond = false;
                for (unsigned i = 0; i < kWcFft; ++i) {
                    const int64_t raw = static_cast<int64_t>(t * kWcHop + i) - 200;
                    const int64_t idx = wc_source_index(c, t, i);
                    if (idx >= 0) any = true;
                    if (raw < 0 || raw >= static_cast<int64_t>(c.P)) mirrored = true;
                    if (raw >= static_cast<int64_t>(c.n_eff)) beyond = true;
                    CHECK(idx < static_cast<int64_t>(c.n_eff), "index past the clip's samples");
                    // numpy.pad(mode = "reflect") of a signal of P samples
                    int64_t want = raw < 0 ? -raw : raw >= static_cast<int64_t>(c.P) ? 2 * (static_cast<int64_t>(c.P) - 1) - raw : raw;
                    if (want >= static_cast<int64_t>(c.n_eff)) want = -1;
                    CHECK(idx == want, "gather rule: pad_to %llu n %llu t %llu i %u", (unsigned long long)pad_to, (unsigned long long)n, (unsigned long long)t, i);
                }
                const WcClass def = !any ? kWcSilent : (!mirrored && !beyond) ? kWcInterior : kWcEdge;
                CHECK(k == def, "class of frame %llu (pad_to %llu, n %llu): %d, by the definition %d", (unsigned long long)t, (unsigned long long)pad_to, (unsigned long long)n, k, def);
            }
            CHECK(count[0] + count[1] + count[2] == c.T && count[0] == c.interior && count[2] == c.T - c.first_silent, "interior + edge + silent = T");
            uint64_t te[kWcMaxEdges];
            CHECK(wc_edges(c, te) == count[1] && count[1] <= kWcMaxEdges, "edge list: %llu edge frames", (unsigned long long)count[1]);
        }
    }

    // ---- the tables of a batch ----
    {
        const uint64_t off[4] = {1000, 7, 50000, 60000}, len[4] = {1120, 399, 9000, 0};
        const WcBatch b = wc_plan(off, len, 0, 4, 0, 80, nullptr, nullptr);
        // clip 0: T = 7 (EEIIIIE); clip 1: T = 0; clip 2: T = 56, interior 2 .. 55 (9000 % 160 = 40: no mirror at the end); clip 3: nothing
        CHECK(b.total_frames == 63 && b.interior_frames == 4 + 54 && b.silent_frames == 0 && b.max_T == 56, "totals %llu %llu", (unsigned long long)b.total_frames, (unsigned long long)b.interior_frames);
        CHECK(b.in_off[0] == 1120 && b.in_frames[0] == 4 && b.in_out_off[0] == 160, "interior of clip 0");
        CHECK(b.in_frames[1] == 0 && b.in_frames[3] == 0, "clips without an interior");
        CHECK(b.in_off[2] == 50120 && b.in_frames[2] == 54 && b.in_out_off[2] == 7 * 80 + 160, "interior of clip 2");
        CHECK(b.records[2].rows_off == 560 && b.records[2].T == 56 && b.records[2].first_silent == 56 && b.rows_floats == 63 * 80, "records");
        CHECK(b.edges.size() == 3 + 2, "edges %zu", b.edges.size());
        const uint64_t want_t[5] = {0, 1, 6, 0, 1}, want_clip[5] = {0, 0, 0, 2, 2};
        for (size_t e = 0; e < b.edges.size() && e < 5; ++e)
            CHECK(b.edges[e].t == want_t[e] && b.edges[e].clip == want_clip[e] && b.edges[e].pcm_off == off[want_clip[e]] &&
                  b.edges[e].row_off == b.records[want_clip[e]].rows_off + want_t[e] * 80, "edge %zu", e);
        // the caller's output offsets: the interior lands two rows in, wherever the clip's rows start
        const uint64_t ro[4] = {4000, 0, 100000, 0};
        const WcBatch r = wc_plan(off, len, 0, 4, 0, 128, ro, nullptr);
        CHECK(r.in_out_off[0] == 4256 && r.in_out_off[2] == 100256 && r.edges[2].row_off == 4000 + 6 * 128, "rows offsets");
        // uniform with pad_to: every clip the same T, silent tails
        const uint64_t one = 2400;
        const WcBatch u = wc_plan(nullptr, &one, 2400, 3, 4800, 80, nullptr, nullptr);
        CHECK(u.total_frames == 90 && u.in_off[2] == 4920 && u.in_frames[2] == 12 && u.records[2].first_silent == 17 && u.silent_frames == 39, "uniform, padded");
    }

    // ---- the argument verdicts, in their order ----
    {
        int x = 0;
        const void *p = &x;
        auto v = [&](bool ctx, bool sup, uint64_t pad, bool rag, uint32_t n, const void *o, const void *l, uint64_t stride, uint64_t len, uint64_t tot, const void *pcm, const void *rows,
                     bool split, const void *mx) { return wc_args(ctx, sup, pad, rag, n, o, l, stride, len, tot, pcm, rows, split, mx); };
        WcArgs a = v(false, false, 7, true, 1, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, true, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && !std::strcmp(a.msg, "ctx is NULL"), "1 ctx");
        a = v(true, false, 7, true, 1, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, true, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_UNSUPPORTED && a.msg == nullptr, "2 support");
        for (uint64_t pad : {uint64_t(1), uint64_t(399)}) {
            a = v(true, true, pad, true, 0, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, true, nullptr);
            CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG, "3 pad_to %llu", (unsigned long long)pad);
        }
        a = v(true, true, 400, true, 0, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, true, nullptr);
        CHECK(a.verdict == kWcDone && a.status == MELSPEC_OK, "4 no clips");
        a = v(true, true, 0, true, 2, p, nullptr, 0, 0, 0, nullptr, nullptr, true, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && !std::strcmp(a.msg, "offset/length array is NULL"), "5 tables");
        a = v(true, true, 0, false, 2, nullptr, nullptr, 100, 400, 4, nullptr, nullptr, false, nullptr);
        CHECK(a.verdict == kWcFail && !std::strcmp(a.msg, "clip_stride smaller than clip_len"), "6 stride");
        a = v(true, true, 0, false, 2, nullptr, nullptr, 0, 400, 4, p, p, false, nullptr);
        CHECK(a.verdict == kWcGo, "stride 0: the same clip n times");
        a = v(true, true, 0, true, 2, p, p, 0, 0, 0, nullptr, nullptr, false, nullptr);
        CHECK(a.verdict == kWcDone, "7 no frames");
        a = v(true, true, 0, true, 2, p, p, 0, 0, 0, nullptr, nullptr, true, p);
        CHECK(a.verdict == kWcSlots, "7 no frames, split: the maxima are still written");
        a = v(true, true, 0, true, 2, p, p, 0, 0, 0, nullptr, nullptr, true, nullptr);
        CHECK(a.verdict == kWcDone, "7 no frames, split without d_clip_max");
        a = v(true, true, 0, true, 2, p, p, 0, 0, 5, nullptr, p, true, nullptr);
        CHECK(a.verdict == kWcFail && !std::strcmp(a.msg, "device pointer is NULL"), "8 pointers before d_clip_max");
        a = v(true, true, 0, true, 2, p, p, 0, 0, 5, p, nullptr, false, nullptr);
        CHECK(a.verdict == kWcFail && !std::strcmp(a.msg, "device pointer is NULL"), "8 rows");
        a = v(true, true, 0, true, 2, p, p, 0, 0, 5, p, p, true, nullptr);
        CHECK(a.verdict == kWcFail && !std::strcmp(a.msg, "d_clip_max is NULL"), "9 d_clip_max");
        a = v(true, true, 480000, true, 2, p, p, 0, 0, 5, p, p, true, p);
        CHECK(a.verdict == kWcGo && a.status == MELSPEC_OK, "go");
    }
    if (bad) { std::printf("whisper_centered_host: %d checks FAILED\n", bad); return 1; }
    std::printf("whisper_centered_host: ok\n");
    return 0;
}
