// blm_stats_host.cpp -- the host side of the NeMo frontend's split output that is arithmetic only (mel_spec_amd/csrc/blm_stats_plan.hpp):
// the order of the argument checks and the plan of a batch -- whole rounds per clip, a block index that fits 32 bits, a scratch size that
// does not overflow -- over the clip lengths of tests/test_blm_split.py and the extremes.  Stand-alone, no HIP, never loaded into Python,
// never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/blm_stats_host.cpp -o /tmp/blm_stats_host && /tmp/blm_stats_host
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

int main() {
    // ---- the plan ----
    const uint64_t cols_list[] = {1, 2, 4, 5, 16, 31, 32, 33, 47, 48, 49, 51, 64, 96, 97, 112, 1001, 1008, 100000, 0xffffffffull, 1ull << 33};
    const uint32_t clips_list[] = {1, 3, 7, 40, 600, 1024, 0xffffffffu};
    for (int f32 = 0; f32 < 2; ++f32)
        for (uint64_t cols : cols_list)
            for (uint32_t n_clips : clips_list)
                for (int nm : {80, 128}) {
                    BlmStatsPlan pl;
                    const bool ok = blm_stats_plan(cols, n_clips, nm, f32 != 0, pl);
                    const uint32_t waves = f32 ? 12u : 8u;
                    CHECK(pl.waves == waves && pl.block_frames == waves * 4, "cols %llu", (unsigned long long)cols);
                    const unsigned __int128 blocks = ((unsigned __int128)cols + pl.block_frames - 1) / pl.block_frames;
                    const bool fits = blocks * n_clips <= 0xffffffffull && blocks * waves <= 0xffffffffull;
                    CHECK(ok == fits, "cols %llu clips %u: ok %d, want %d", (unsigned long long)cols, n_clips, (int)ok, (int)fits);
                    if (!ok) continue;
                    CHECK(pl.blocks_per_clip == (uint64_t)blocks, "blocks %u", pl.blocks_per_clip);
                    CHECK(pl.units_per_clip == pl.blocks_per_clip * waves && pl.units_per_clip % waves == 0, "units %u", pl.units_per_clip);
                    CHECK((uint64_t)pl.units_per_clip * 4 >= cols && (uint64_t)(pl.units_per_clip - waves) * 4 < cols, "units %u do not cover %llu columns tightly", pl.units_per_clip, (unsigned long long)cols);
                    CHECK(pl.n_units == (uint64_t)pl.units_per_clip * n_clips && pl.n_units / waves <= 0xffffffffull, "n_units");
                    CHECK(pl.part_bytes == (uint64_t)(blocks * n_clips) * nm * 8, "part_bytes");
                    // every valid frame falls into exactly one block, in order
                    if (cols <= 100000) {
                        uint64_t covered = 0;
                        for (uint32_t b = 0; b < pl.blocks_per_clip; ++b) {
                            const uint64_t left = cols > (uint64_t)b * pl.block_frames ? cols - (uint64_t)b * pl.block_frames : 0;
                            covered += left < pl.block_frames ? left : pl.block_frames;
                        }
                        CHECK(covered == cols, "blocks cover %llu of %llu frames", (unsigned long long)covered, (unsigned long long)cols);
                    }
                }
    BlmStatsPlan pl;
    CHECK(!blm_stats_plan(0, 1, 80, false, pl) && !blm_stats_plan(10, 0, 80, false, pl) && !blm_stats_plan(10, 1, 0, false, pl), "degenerate batches have no plan");
    CHECK(!blm_stats_plan(~0ull, 1, 128, true, pl), "2^64 - 1 columns");

    // ---- the argument checks, in their order ----
    int x = 0;
    const void *p = &x;
    BlmStatsArgs a = blm_stats_args(false, false, 1, 10, p, p, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strcmp(a.msg, "blm is NULL") == 0, "null context");
    a = blm_stats_args(true, false, 0, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_UNSUPPORTED && a.msg == nullptr, "an unsupported context is refused before anything else is looked at");
    a = blm_stats_args(true, true, 0, 10, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsDone && a.status == MELSPEC_OK, "no clips");
    a = blm_stats_args(true, true, 5, 0, nullptr, nullptr, nullptr, nullptr);
    CHECK(a.verdict == kBlmStatsDone && a.status == MELSPEC_OK, "no valid frame: OK, nothing written, the pointers are not looked at");
    a = blm_stats_args(true, true, 5, 10, nullptr, p, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG, "d_pcm NULL");
    a = blm_stats_args(true, true, 5, 10, p, nullptr, p, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG, "d_rows NULL");
    a = blm_stats_args(true, true, 5, 10, p, p, nullptr, p);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg, "d_mean NULL");
    a = blm_stats_args(true, true, 5, 10, p, p, p, nullptr);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg, "d_inv_std NULL");
    a = blm_stats_args(true, true, 5, 10, p, p, p, p);
    CHECK(a.verdict == kBlmStatsGo && a.status == MELSPEC_OK, "go");

    if (bad) { std::printf("blm_stats_host: %d checks failed\n", bad); return 1; }
    std::printf("blm_stats_host: ok\n");
    return 0;
}
