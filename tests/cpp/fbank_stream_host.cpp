// The Kaldi fbank stream bank's bookkeeping (mel_spec_amd/csrc/fbank_stream_plan.hpp) on the host: the bank's slots are a float array,
// scatter and carry are the loops of the kernels in aux_kernels.hpp, and the frame kernel's place is taken by the CPU oracle's
// Fbank::compute on each entry's span of the state.  Rows are prefix-stable and a row depends on its own samples (and, for non-finite
// input only, the one in front), so every stream's concatenated rows must be the oracle's rows of its concatenated samples, bit for bit.
// Linked against oracle/libmelspec_oracle.so.  Prints "fbank_stream_host: ok" and the first-push counts; exit status 1 on any mismatch.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "fbank_stream_plan.hpp"
#include "fused512_route.hpp"

extern "C" {
typedef struct {
    double sample_rate;
    int num_mel_bins;
    double frame_length_ms, frame_shift_ms, energy_floor;
    int use_log_fbank, use_power;
    double preemphasis;
    int apply_cmn;
    double low_freq, high_freq;
} oracle_fbank_config;
void oracle_fbank_default_config(oracle_fbank_config *c);
int oracle_fbank_frame_length(const oracle_fbank_config *c);
int oracle_fbank_frame_shift(const oracle_fbank_config *c);
int64_t oracle_fbank_compute(const oracle_fbank_config *cfg, const float *samples, int64_t len, float *out);
}

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
static float noise() { return (static_cast<float>(rnd() & 0xffff) - 32768.0f) * (0.4f / 32768.0f); }

struct HostBank {
    oracle_fbank_config cfg;
    FbankStreamGeom g;
    FbankStreamBook bk;
    std::vector<float> state;
    HostBank(int shift, uint32_t n_streams, uint32_t max_chunk) {
        oracle_fbank_default_config(&cfg);
        cfg.apply_cmn = 0;
        cfg.frame_shift_ms = shift * 1000.0 / 16000.0;
        g = fbank_stream_geometry(static_cast<uint32_t>(oracle_fbank_frame_length(&cfg)), static_cast<uint32_t>(oracle_fbank_frame_shift(&cfg)), 80, n_streams, max_chunk);
        bk.reset(n_streams);
        // what a slot held before: never zero, so a row that reads in front of its stream's samples shows
        state.assign(static_cast<size_t>(n_streams) * g.stride, 1.0e6f);
    }
    // 0 or the plan's error code; rows: the entries' rows back to back
    int push(const std::vector<uint32_t> &ids, const std::vector<std::vector<float>> &chunks, std::vector<float> &rows, FbankStreamPlan &pl) {
        std::vector<uint32_t> lens;
        for (const auto &c : chunks) lens.push_back(static_cast<uint32_t>(c.size()));
        const char *err = "";
        const uint32_t n = static_cast<uint32_t>(ids.size());
        if (const int rc = fbank_stream_plan_push(g, bk, ids.data(), lens.data(), n, pl, &err)) return rc;
        rows.assign(pl.total_frames * g.n_mels, 0.0f);
        for (uint32_t i = 0; i < n; ++i) {                // scatter
            const StreamEntry &e = pl.entries[i];
            if (e.len) std::memcpy(&state[e.stream * g.stride + g.in_off], chunks[i].data(), e.len * sizeof(float));
        }
        for (uint32_t i = 0; i < n; ++i) {                // frames
            if (!pl.frames[i]) continue;
            const int64_t span = static_cast<int64_t>(pl.frames[i] - 1) * g.shift + g.frame_len;
            const int64_t got = oracle_fbank_compute(&cfg, &state[pl.off[i]], span, &rows[pl.out_off[i]]);
            CHECK(got == static_cast<int64_t>(pl.frames[i]), "oracle frames %" PRId64 " != %" PRIu64, got, pl.frames[i]);
        }
        for (uint32_t i = 0; i < n; ++i) {                // carry
            const StreamEntry &e = pl.entries[i];
            if (!e.len) continue;
            float *slot = &state[e.stream * g.stride];
            std::memmove(slot + g.in_off - e.keep, slot + g.in_off + e.len - e.keep, e.keep * sizeof(float));
        }
        fbank_stream_commit_push(g, bk, ids.data(), lens.data(), n);
        return 0;
    }
};

static void drive(int shift, uint32_t max_chunk) {
    const uint32_t n_streams = 5, frame_len = 400;
    const uint32_t target = shift == 1 ? 1500 : 7000;
    HostBank b(shift, n_streams, max_chunk);
    CHECK(b.g.shift == static_cast<uint32_t>(shift) && b.g.frame_len == frame_len && b.g.in_off >= frame_len + 1 && b.g.in_off % 4 == 0, "geometry of shift %d", shift);
    std::vector<std::vector<float>> src(n_streams), got(n_streams);
    for (auto &s : src) { s.resize(target); for (auto &v : s) v = noise(); }
    std::vector<uint32_t> pos(n_streams, 0);
    const uint32_t sizes[12] = {0, 1, static_cast<uint32_t>(shift - 1), static_cast<uint32_t>(shift), static_cast<uint32_t>(shift + 1), 239, 240, 241, 399, 400, 401, max_chunk};
    uint32_t live = n_streams;
    while (live) {
        std::vector<uint32_t> ids;
        std::vector<std::vector<float>> chunks;
        for (uint32_t s = 0; s < n_streams; ++s) {
            if (pos[s] >= target || rnd() % 10 >= 7) continue;
            uint32_t len = sizes[rnd() % 12];
            if (len > max_chunk) len = max_chunk;
            if (len > target - pos[s]) len = target - pos[s];
            ids.push_back(s);
            chunks.emplace_back(src[s].begin() + pos[s], src[s].begin() + pos[s] + len);
        }
        if (ids.empty()) continue;
        std::vector<size_t> want;
        for (size_t i = 0; i < ids.size(); ++i) want.push_back(fbank_stream_frames_after(b.g, b.bk, ids[i], static_cast<uint32_t>(chunks[i].size())));
        std::vector<float> rows;
        FbankStreamPlan pl;
        const std::vector<uint64_t> emitted_before = b.bk.emitted;
        const std::vector<uint32_t> pending_before = b.bk.pending;
        CHECK(b.push(ids, chunks, rows, pl) == 0, "push failed");
        for (size_t i = 0; i < ids.size(); ++i) {
            const uint32_t s = ids[i];
            const StreamEntry &e = pl.entries[i];
            CHECK(pl.frames[i] == want[i] && e.frames == want[i], "frames_after %zu, push %" PRIu64, want[i], pl.frames[i]);
            CHECK(pl.continues[i] == (emitted_before[s] > 0 ? 1u : 0u), "continues flag of stream %u", s);
            CHECK(e.keep <= frame_len && e.stream == s && e.len == chunks[i].size(), "entry of stream %u: keep %u", s, e.keep);
            CHECK(pl.off[i] == s * b.g.stride + b.g.in_off - pending_before[s], "span of stream %u", s);
            pos[s] += e.len;
            got[s].insert(got[s].end(), rows.begin() + pl.out_off[i], rows.begin() + pl.out_off[i] + pl.frames[i] * b.g.n_mels);
            // after the carry: the slot ends with the samples from emitted * shift - 1 (the predecessor, once a frame is out) on
            const uint64_t em = b.bk.emitted[s], first = em ? em * shift - 1 : 0;
            const uint32_t held = static_cast<uint32_t>(pos[s] - first);
            CHECK(b.bk.total[s] == pos[s] && b.bk.pending[s] + (em ? 1u : 0u) == held && (e.len == 0 || e.keep == held), "book of stream %u", s);
            if (e.len)
                CHECK(std::memcmp(&b.state[s * b.g.stride + b.g.in_off - held], &src[s][first], held * sizeof(float)) == 0, "carry of stream %u after %u samples", s, pos[s]);
            if (pos[s] >= target) --live;
        }
    }
    std::vector<float> want;
    for (uint32_t s = 0; s < n_streams; ++s) {
        const uint64_t frames = fbank_stream_frames(b.g, target);
        want.assign(frames * b.g.n_mels, 0.0f);
        CHECK(oracle_fbank_compute(&b.cfg, src[s].data(), target, want.data()) == static_cast<int64_t>(frames), "oracle frames");
        CHECK(got[s].size() == want.size(), "shift %d chunk %u stream %u: %zu values, want %zu", shift, max_chunk, s, got[s].size(), want.size());
        if (got[s].size() == want.size())
            CHECK(std::memcmp(got[s].data(), want.data(), want.size() * sizeof(float)) == 0, "shift %d chunk %u stream %u: rows differ from Fbank::compute", shift, max_chunk, s);
    }
}

int main() {
    for (int shift : {160, 120, 400, 1})
        for (uint32_t max_chunk : {160u, 517u, 2000u}) drive(shift, max_chunk);
    // first pushes of 160 samples: the reference needs 400, then one frame per shift
    {
        HostBank b(160, 1, 160);
        std::printf("first_pushes");
        for (int k = 0; k < 5; ++k) {
            std::vector<float> rows;
            FbankStreamPlan pl;
            std::vector<float> c(160);
            for (auto &v : c) v = noise();
            CHECK(b.push({0}, {c}, rows, pl) == 0, "push failed");
            std::printf(" %" PRIu64, pl.frames[0]);
        }
        std::printf("\n");
    }
    // refusals leave the book as it was
    {
        HostBank b(160, 3, 100);
        std::vector<float> rows, z(10, 0.0f);
        FbankStreamPlan pl;
        CHECK(b.push({0, 1}, {z, z}, rows, pl) == 0, "push failed");
        const FbankStreamBook before = b.bk;
        CHECK(b.push({3}, {z}, rows, pl) == 1, "id out of range");
        CHECK(b.push({1, 1}, {z, z}, rows, pl) == 1, "an id twice in one push");
        CHECK(b.push({0, 2}, {z, std::vector<float>(101, 0.0f)}, rows, pl) == 2, "chunk longer than max_chunk");
        CHECK(b.bk.total == before.total && b.bk.emitted == before.emitted && b.bk.pending == before.pending, "a refused push changed the book");
        CHECK(fbank_stream_frames_after(b.g, b.bk, 0, 100) == 0 && fbank_stream_frames_after(b.g, b.bk, 0, 390) == 1, "frames_after");
    }
    // the stream kernel of an object is its plain batch's kernel with the flag: same waves, run form, slot lengths, LDS and grid rule --
    // what the bit identity of a stream's rows with the batch call rests on; no other flavour and no object off the fused path has one
    {
        using namespace melspec::host;
        for (Bank512 bank : {Bank512::kKaldi80, Bank512::kKaldi40, Bank512::kRuntime, Bank512::kSlaney80})
            for (int waves : {8, 4})
                for (bool fused : {true, false}) {
                    const Fused512Shape s{Flavor512::kKaldi, fused, bank, true, waves, false, MELSPEC_PRECISION_F64, false, false, false};
                    const Launch512 a = route512(s, Batch512::kPlain).run, b = route512(s, Batch512::kStream).run;
                    if (!fused) { CHECK(b.kernel == K512::kNone, "a stream kernel off the fused path"); continue; }
                    const K512Info ia = info_of(a.kernel), ib = info_of(b.kernel);
                    CHECK(is_stream(b.kernel) && !is_stream(a.kernel) && is_fast(a.kernel), "stream route of bank %d on %d waves", static_cast<int>(bank), waves);
                    CHECK(ia.waves == ib.waves && ia.f32 == ib.f32 && ia.runs == ib.runs && ia.rt_lens == ib.rt_lens, "stream kernel's shape, bank %d on %d waves", static_cast<int>(bank), waves);
                    CHECK(a.waves == b.waves && a.lds == b.lds && a.units_per_group == b.units_per_group && a.lab_per_cu == b.lab_per_cu, "stream launch, bank %d on %d waves", static_cast<int>(bank), waves);
                }
        for (Flavor512 f : {Flavor512::kNemo, Flavor512::kWhisper}) {
            const Fused512Shape s{f, true, Bank512::kSlaney80, true, 8, true, MELSPEC_PRECISION_F64, false, false, false};
            CHECK(route512(s, Batch512::kStream).run.kernel == K512::kNone, "a stream kernel of another flavour");
        }
        CHECK(static_cast<int>(K512::kEnd) - static_cast<int>(K512::kStream80) == 4 && K512::kStream80 == K512::kCount, "four stream kernels behind the batch kernels");
    }
    if (g_failures) { std::printf("fbank_stream_host: %d failures\n", g_failures); return 1; }
    std::printf("fbank_stream_host: ok\n");
    return 0;
}
