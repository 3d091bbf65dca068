// blm_stats_ragged_host.cpp -- the host side of the split output's ragged form (melspec_blm_compute_ragged_device_split) that is
// arithmetic only (mel_spec_amd/csrc/blm_stats_plan.hpp): blm_stats_plan_ragged, the unit count plan_ragged gives a clip, and the order
// of the argument checks.  What it pins first is the invariant the kernels' waits rest on -- EVERY clip's unit count, and so the batch's,
// is a multiple of the kernel's waves: RoundStats::wait_free and StagedRows::wait_staged wait for every wave of a round, and a round
// with a wave missing never ends.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/blm_stats_ragged_host.cpp -o /tmp/blm_stats_ragged_host && /tmp/blm_stats_ragged_host
#include <cstdio>
#include <cstring>
#include <vector>

#include "blm_stats_plan.hpp"

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

int main() {
    const uint64_t edge_cols[] = {0, 1, 31, 32, 33, 47, 48, 49, 97, 0, 2, 4, 5, 16, 64, 96, 112, 1001, 1008};
    const size_t n_edge = sizeof(edge_cols) / sizeof(edge_cols[0]);

    // ---- random batches: empty clips, the widths where a block of either kernel ends, both waves values ----
    for (int f32 = 0; f32 < 2; ++f32)
        for (int trial = 0; trial < 400; ++trial) {
            const uint32_t waves = f32 ? 12u : 8u, bf = waves * 4;
            const uint32_t n_clips = 1 + lcg() % 40;
            const int nm = (trial & 1) ? 128 : 80;
            std::vector<uint64_t> cols(n_clips);
            for (auto &c : cols) c = (lcg() % 4 == 0) ? lcg() % 3000 : edge_cols[lcg() % n_edge];
            if (trial == 0) cols.assign(edge_cols, edge_cols + n_edge);           // every edge width at least once, in one batch
            const uint32_t n = static_cast<uint32_t>(cols.size());
            std::vector<uint64_t> prefix(n + 1, ~0ull);
            BlmStatsRaggedPlan pl;
            const bool ok = blm_stats_plan_ragged(cols.data(), n, nm, f32 != 0, pl, prefix.data());
            CHECK(pl.waves == waves && pl.block_frames == bf, "trial %d", trial);
            uint64_t total_blocks = 0, total_units = 0, any = 0;
            for (uint32_t c = 0; c < n; ++c) {
                const uint64_t blocks_c = (cols[c] + bf - 1) / bf;               // ceil(cols_c / block_frames), 0 for an empty clip
                const uint64_t units_c = ragged_clip_units(cols[c], kBlmStatsFramesPerUnit, waves);       // what plan_ragged gives the clip
                CHECK(blm_stats_blocks(cols[c], bf) == blocks_c, "clip %u: cols %llu", c, (unsigned long long)cols[c]);
                CHECK(units_c % waves == 0, "clip %u: %llu units are no multiple of %u waves", c, (unsigned long long)units_c, waves);
                CHECK(units_c == blocks_c * waves, "clip %u: %llu units, %llu blocks", c, (unsigned long long)units_c, (unsigned long long)blocks_c);
                CHECK(units_c * 4 >= cols[c] && (units_c == 0 ? cols[c] == 0 : (units_c - waves) * 4 < cols[c]), "clip %u: units do not cover the row tightly", c);
                CHECK((cols[c] == 0) == (units_c == 0), "clip %u: an empty clip has no unit, any other has one", c);
                CHECK(prefix[c] == total_blocks, "clip %u: block prefix %llu, want %llu", c, (unsigned long long)prefix[c], (unsigned long long)total_blocks);
                CHECK(total_units % waves == 0 && total_units / waves == prefix[c], "clip %u: unit_prefix / waves is the clip's first block", c);
                total_blocks += blocks_c;
                total_units += units_c;
                any |= cols[c];
            }
            CHECK(ok == (any != 0), "trial %d: ok %d", trial, (int)ok);
            CHECK(prefix[n] == total_blocks, "the prefix ends at the batch's blocks");
            if (!ok) continue;
            CHECK(pl.n_blocks == total_blocks, "n_blocks %u, want %llu", pl.n_blocks, (unsigned long long)total_blocks);
            CHECK(pl.n_units == (uint64_t)waves * total_blocks && pl.n_units == total_units && pl.n_units % waves == 0, "n_units %llu", (unsigned long long)pl.n_units);
            CHECK(pl.part_bytes == total_blocks * (uint64_t)nm * 8, "part_bytes %llu", (unsigned long long)pl.part_bytes);
        }

    // ---- a one-clip batch is blm_stats_plan's batch of that clip ----
    for (int f32 = 0; f32 < 2; ++f32)
        for (uint64_t cols : edge_cols)
            for (int nm : {80, 128}) {
                if (cols == 0) continue;
                BlmStatsPlan one;
                BlmStatsRaggedPlan pl;
                CHECK(blm_stats_plan(cols, 1, nm, f32 != 0, one) && blm_stats_plan_ragged(&cols, 1, nm, f32 != 0, pl), "cols %llu", (unsigned long long)cols);
                CHECK(pl.waves == one.waves && pl.block_frames == one.block_frames && pl.n_blocks == one.blocks_per_clip && pl.n_units == one.n_units &&
                      pl.n_units == one.units_per_clip && pl.part_bytes == one.part_bytes, "cols %llu: the one-clip ragged plan differs from the uniform plan", (unsigned long long)cols);
                CHECK(ragged_clip_units(cols, kBlmStatsFramesPerUnit, one.waves) == one.units_per_clip, "cols %llu: plan_ragged's units", (unsigned long long)cols);
            }
    // round_units = 1: the table every other caller of plan_ragged gets
    for (uint64_t fr : {0ull, 1ull, 3ull, 4ull, 5ull, 1001ull, (1ull << 40) + 1})
        for (uint32_t fpu : {1u, 4u, 5u, 6u})
            CHECK(ragged_clip_units(fr, fpu, 1) == (fr + fpu - 1) / fpu && ragged_clip_units(fr, fpu, 0) == (fr + fpu - 1) / fpu, "frames %llu per %u", (unsigned long long)fr, fpu);

    // ---- what does not fit ----
    BlmStatsRaggedPlan pl;
    {
        uint64_t c1 = 10;
        CHECK(!blm_stats_plan_ragged(nullptr, 1, 80, false, pl) && !blm_stats_plan_ragged(&c1, 0, 80, false, pl) && !blm_stats_plan_ragged(&c1, 1, 0, false, pl), "degenerate batches have no plan");
        const uint64_t none[3] = {0, 0, 0};
        CHECK(!blm_stats_plan_ragged(none, 3, 80, false, pl), "a batch without a column has no plan");
        // 2^32 - 1 blocks fit the kernels' 32-bit count, 2^32 do not -- in one clip or spread over many
        for (int f32 = 0; f32 < 2; ++f32) {
            const uint64_t bf = f32 ? 48 : 32;
            uint64_t c = 0xffffffffull * bf;
            CHECK(blm_stats_plan_ragged(&c, 1, 80, f32 != 0, pl) && pl.n_blocks == 0xffffffffu && pl.n_units == 0xffffffffull * (bf / 4), "2^32 - 1 blocks");
            CHECK(pl.part_bytes == 0xffffffffull * 80 * 8, "their scratch");
            c += 1;
            CHECK(!blm_stats_plan_ragged(&c, 1, 80, f32 != 0, pl), "2^32 blocks in one clip");
            const uint64_t many[4] = {0x40000000ull * bf, 0x40000000ull * bf, 0x40000000ull * bf, 0x40000000ull * bf};
            CHECK(!blm_stats_plan_ragged(many, 4, 80, f32 != 0, pl), "2^32 blocks over four clips");
            const uint64_t fewer[4] = {0x40000000ull * bf, 0x40000000ull * bf, 0x40000000ull * bf, 0x40000000ull * bf - bf};
            CHECK(blm_stats_plan_ragged(fewer, 4, 80, f32 != 0, pl) && pl.n_blocks == 0xffffffffu, "2^32 - 1 blocks over four clips");
            const uint64_t huge[2] = {~0ull, ~0ull};
            CHECK(!blm_stats_plan_ragged(huge, 2, 128, f32 != 0, pl), "2^64 - 1 columns twice: no wrap");
        }
        // the scratch: blocks * n_mels * 8 bytes (+ 16) has to fit size_t
        if (sizeof(size_t) == 8) {
            uint64_t c = 0xffffffffull * 32;
            CHECK(!blm_stats_plan_ragged(&c, 1, 0x7fffffff, false, pl), "2^32 blocks x 2^31 rows x 8 bytes is past size_t");
            CHECK(blm_stats_plan_ragged(&c, 1, 1 << 20, false, pl) && pl.part_bytes == 0xffffffffull * (1ull << 20) * 8, "2^55 bytes still count");
        }
    }

    // ---- the argument checks, in the order of melspec_blm_compute_ragged_device ----
    int x = 0;
    const void *p = &x;
    BlmStatsArgs a = blm_stats_ragged_args(false, false, 1, p, p, 10, p, p, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strcmp(a.msg, "blm is NULL") == 0, "null context");
    a = blm_stats_ragged_args(true, false, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_UNSUPPORTED && a.msg == nullptr, "an unsupported context is refused before anything else is looked at");
    a = blm_stats_ragged_args(true, true, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsDone && a.status == MELSPEC_OK, "no clips: OK before the tables are looked at");
    a = blm_stats_ragged_args(true, true, 3, nullptr, p, 10, p, p, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "offset/length"), "h_offsets NULL");
    a = blm_stats_ragged_args(true, true, 3, p, nullptr, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "offset/length"), "h_lengths NULL comes before 'nothing to do'");
    a = blm_stats_ragged_args(true, true, 3, p, p, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsDone && a.status == MELSPEC_OK, "no valid frame: OK, nothing written, the device pointers are not looked at");
    a = blm_stats_ragged_args(true, true, 3, p, p, 10, nullptr, p, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strcmp(a.msg, "device pointer is NULL") == 0, "d_pcm NULL");
    a = blm_stats_ragged_args(true, true, 3, p, p, 10, p, nullptr, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strcmp(a.msg, "device pointer is NULL") == 0, "d_rows NULL");
    a = blm_stats_ragged_args(true, true, 3, p, p, 10, p, p, nullptr, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "d_mean"), "d_mean NULL");
    a = blm_stats_ragged_args(true, true, 3, p, p, 10, p, p, p, nullptr);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "d_inv_std"), "d_inv_std NULL");
    a = blm_stats_ragged_args(true, true, 3, p, p, 10, p, p, p, p);
    CHECK(a.verdict == kBlmStatsGo && a.status == MELSPEC_OK, "go");

    if (bad) { std::printf("blm_stats_ragged_host: %d checks failed\n", bad); return 1; }
    std::printf("blm_stats_ragged_host: ok\n");
    return 0;
}
