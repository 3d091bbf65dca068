// blm_split_io_host.cpp -- the host side of the split output with 16-bit ends (melspec_blm_compute_*_split_io) that is arithmetic only
// (mel_spec_amd/csrc/blm_split_io_plan.hpp): the dtype codes, the order of the argument checks -- the f32 split calls' own, the codes in
// front and the alignment behind the NULL checks -- and the index of a kernel in the side table of fbank512_stats_io.hip.  Stand-alone,
// no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/blm_split_io_host.cpp -o /tmp/blm_split_io_host && /tmp/blm_split_io_host
#include <cstdio>
#include <cstring>
#include <set>

#include "blm_split_io_plan.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

static bool same(const BlmStatsArgs &a, const BlmStatsArgs &b) {
    return a.verdict == b.verdict && a.status == b.status && ((a.msg == nullptr) == (b.msg == nullptr)) && (!a.msg || !std::strcmp(a.msg, b.msg));
}

int main() {
    // ---- the side table: four stats kernels x five combinations, every slot once, in the order of io_index ----
    static_assert(kBlmSplitIoStatsKernels == 4 && kBlmSplitIoCombos == 5 && kBlmSplitIoKernels == 20, "MS_K512_STATS x MS_IO_COMBOS");
    const K512 stats[] = {K512::kStats128, K512::kStats80, K512::kStats128F32, K512::kStats80F32};
    std::set<int> seen;
    for (int k = 0; k < 4; ++k)
        for (int pcm = 0; pcm <= 1; ++pcm)
            for (int out = 0; out <= 2; ++out) {
                const int io = pcm | out << 4, at = blm_split_io_slot(stats[k], io);
                if (io == 0) {
                    CHECK(at < 0, "(F32, F32) is the existing kernels': no slot, got %d", at);
                    continue;
                }
                CHECK(at == k * 5 + io_index(io), "kernel %d io %#x: slot %d", k, io, at);
                CHECK(at >= 0 && at < kBlmSplitIoKernels && seen.insert(at).second, "kernel %d io %#x: slot %d out of range or taken twice", k, io, at);
            }
    CHECK(seen.size() == 20, "%zu slots", seen.size());
    // what is no stats kernel, or no combination, has no slot
    for (int k = static_cast<int>(K512::kNone); k < static_cast<int>(K512::kEnd); ++k) {
        const K512 kk = static_cast<K512>(k);
        if (!is_stats(kk)) CHECK(blm_split_io_slot(kk, MELSPEC_PCM_S16 | MELSPEC_OUT_F16 << 4) < 0, "K512 %d is no stats kernel", k);
    }
    for (int io : {-1, 0, 2, 3, 1 | 3 << 4, 2 | 1 << 4, 0x100, 0x7fffffff})
        CHECK(blm_split_io_slot(K512::kStats80, io) < 0, "io %#x is no combination", io);
    // the f32 kernels' slots follow the f64 kernels': the launch shape comes from the stats kernel, not from the slot
    CHECK(info_of(K512::kStats128).waves == 8 && info_of(K512::kStats80F32).waves == 12 && info_of(K512::kStats80F32).f32, "the stats kernels' shapes");

    // ---- the dtype codes: in front of everything but the NULL context ----
    int io = -7;
    BlmStatsArgs a = blm_split_io_codes(false, 99, 99, io);
    CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "blm is NULL") && io == 0, "NULL context first");
    for (int pcm = -2; pcm <= 3; ++pcm)
        for (int out = -2; out <= 4; ++out) {
            a = blm_split_io_codes(true, pcm, out, io);
            const bool pk = pcm == MELSPEC_PCM_F32 || pcm == MELSPEC_PCM_S16, ok = out == MELSPEC_OUT_F32 || out == MELSPEC_OUT_F16 || out == MELSPEC_OUT_BF16;
            if (pk && ok) {
                CHECK(a.verdict == kBlmStatsGo && a.status == MELSPEC_OK && io == (pcm | out << 4), "(%d, %d)", pcm, out);
            } else {
                CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, pk ? "out_dtype" : "pcm_dtype") && io == 0,
                      "(%d, %d): %s", pcm, out, a.msg ? a.msg : "(null)");
            }
        }

    // ---- the arguments: the f32 split call's verdicts in its order, then the alignment of the typed pointers ----
    alignas(16) static char buf[64];
    const void *even = buf, *odd = buf + 1, *two = buf + 2;
    const int combos[] = {MELSPEC_PCM_S16 | MELSPEC_OUT_F32 << 4, MELSPEC_PCM_F32 | MELSPEC_OUT_F16 << 4, MELSPEC_PCM_F32 | MELSPEC_OUT_BF16 << 4,
                          MELSPEC_PCM_S16 | MELSPEC_OUT_F16 << 4, MELSPEC_PCM_S16 | MELSPEC_OUT_BF16 << 4};
    for (int c : combos) {
        const bool s16 = (c & 15) == MELSPEC_PCM_S16, half = (c >> 4) != MELSPEC_OUT_F32;
        for (int sup = 0; sup < 2; ++sup)
            for (uint32_t n_clips = 0; n_clips < 2; ++n_clips)
                for (uint64_t cols = 0; cols < 2; ++cols)
                    for (int nulls = 0; nulls < 16; ++nulls) {
                        const void *pcm = (nulls & 1) ? nullptr : even, *rows = (nulls & 2) ? nullptr : even, *mean = (nulls & 4) ? nullptr : even, *inv = (nulls & 8) ? nullptr : even;
                        const BlmStatsArgs want = blm_stats_args(true, sup != 0, n_clips, cols, pcm, rows, mean, inv);
                        CHECK(same(blm_split_io_args(sup != 0, n_clips, cols, pcm, rows, mean, inv, c), want), "uniform io %#x sup %d clips %u cols %llu nulls %d", c, sup,
                              n_clips, (unsigned long long)cols, nulls);
                        for (int tabs = 0; tabs < 4; ++tabs) {
                            const void *offs = (tabs & 1) ? nullptr : even, *lens = (tabs & 2) ? nullptr : even;
                            const BlmStatsArgs rwant = blm_stats_ragged_args(true, sup != 0, n_clips, offs, lens, cols, pcm, rows, mean, inv);
                            CHECK(same(blm_split_io_ragged_args(sup != 0, n_clips, offs, lens, cols, pcm, rows, mean, inv, c), rwant), "ragged io %#x sup %d clips %u cols %llu nulls %d tabs %d",
                                  c, sup, n_clips, (unsigned long long)cols, nulls, tabs);
                        }
                    }
        // alignment: natural alignment of the element type is enough, and is asked for -- behind every other check
        const struct { const void *pcm, *rows; bool bad; } cases[] = {
            {even, even, false}, {two, two, !s16 || !half}, {odd, even, true}, {even, odd, true}, {two, even, !s16}, {even, two, !half}};
        for (const auto &k : cases) {
            a = blm_split_io_args(true, 1, 1, k.pcm, k.rows, even, even, c);
            CHECK((a.verdict == kBlmStatsFail) == k.bad && (!k.bad || (a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "aligned"))), "uniform io %#x alignment", c);
            a = blm_split_io_ragged_args(true, 1, even, even, 1, k.pcm, k.rows, even, even, c);
            CHECK((a.verdict == kBlmStatsFail) == k.bad && (!k.bad || (a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "aligned"))), "ragged io %#x alignment", c);
            // ... and not looked at where the call has nothing to do or does not support the context
            CHECK(blm_split_io_args(true, 0, 1, k.pcm, k.rows, even, even, c).verdict == kBlmStatsDone, "no clips: done");
            CHECK(blm_split_io_args(true, 1, 0, k.pcm, k.rows, even, even, c).verdict == kBlmStatsDone, "no columns: done");
            a = blm_split_io_args(false, 1, 1, k.pcm, k.rows, even, even, c);
            CHECK(a.verdict == kBlmStatsFail && a.status == MELSPEC_ERR_UNSUPPORTED && a.msg == nullptr, "unsupported first, worded by the caller");
        }
    }
    CHECK(blm_split_io_pcm_bytes(MELSPEC_PCM_S16) == 2 && blm_split_io_pcm_bytes(MELSPEC_PCM_F32) == 4 && blm_split_io_out_bytes(MELSPEC_OUT_F32) == 4 &&
          blm_split_io_out_bytes(MELSPEC_OUT_F16) == 2 && blm_split_io_out_bytes(MELSPEC_OUT_BF16) == 2, "element sizes");

    if (bad) {
        std::printf("blm_split_io_host: %d checks FAILED\n", bad);
        return 1;
    }
    std::printf("blm_split_io_host: ok\n");
    return 0;
}
