// fbank_split_io_host.cpp -- the host side of the Kaldi fbank's split output for ragged batches and with 16-bit ends
// (melspec_fbank_compute_ragged_device_split, melspec_fbank_compute_*_split_io) that is arithmetic only
// (mel_spec_amd/csrc/fbank_split_io_plan.hpp): the dtype codes and the io code, the order of the argument checks against a literal table,
// and the index of a kernel in the side table of fbank512_kaldi_split_io.hip -- ten kernels, every slot once.  Stand-alone, no HIP, never
// loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/fbank_split_io_host.cpp -o /tmp/fbank_split_io_host && /tmp/fbank_split_io_host
#include <cstdio>
#include <cstring>
#include <set>

#include "fbank_split_io_plan.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

int main() {
    // ---- the io codes and the side table: two kinds of batch x five combinations, every slot once ----
    static_assert(kFbankSplitIoCombos == 5 && kFbankSplitIoKernels == 10, "{uniform, ragged} x MS_IO_COMBOS");
    // (pcm, out) -> io, slot of the uniform kernel; the ragged kernel's is five further on
    const struct { int pcm, out, io, slot; } table[] = {
        {MELSPEC_PCM_F32, MELSPEC_OUT_F32, 0x00, -1}, {MELSPEC_PCM_F32, MELSPEC_OUT_F16, 0x10, 0}, {MELSPEC_PCM_F32, MELSPEC_OUT_BF16, 0x20, 1},
        {MELSPEC_PCM_S16, MELSPEC_OUT_F32, 0x01, 2},  {MELSPEC_PCM_S16, MELSPEC_OUT_F16, 0x11, 3}, {MELSPEC_PCM_S16, MELSPEC_OUT_BF16, 0x21, 4}};
    std::set<int> seen;
    for (const auto &t : table) {
        int io = -7;
        const FbankSplitArgs a = fbank_split_io_codes(true, t.pcm, t.out, io);
        CHECK(a.verdict == kFbankSplitGo && a.status == MELSPEC_OK && io == t.io, "(%d, %d): io %#x", t.pcm, t.out, io);
        for (int ragged = 0; ragged < 2; ++ragged) {
            const int at = fbank_split_io_slot(ragged != 0, io);
            if (t.slot < 0) {
                CHECK(at < 0, "(F32, F32) is the f32 split calls': no slot, got %d", at);
                continue;
            }
            CHECK(at == t.slot + 5 * ragged, "io %#x ragged %d: slot %d", io, ragged, at);
            CHECK(at >= 0 && at < kFbankSplitIoKernels && seen.insert(at).second, "io %#x ragged %d: slot %d out of range or taken twice", io, ragged, at);
        }
    }
    CHECK(seen.size() == 10, "%zu slots", seen.size());
    for (int io : {-1, 0, 2, 3, 1 | 3 << 4, 2 | 1 << 4, 0x100, 0x7fffffff})
        CHECK(fbank_split_io_slot(false, io) < 0 && fbank_split_io_slot(true, io) < 0, "io %#x is no combination", io);
    // the launch shape is the f32 clip kernel's of the same kind of batch: eight waves, the f64 LDS plus the CMN block, one workgroup per CU
    {
        Fused512Shape s{Flavor512::kKaldi, true, Bank512::kKaldi80, true, 8, false, MELSPEC_PRECISION_F64, false, false, true};
        CHECK(fbank_split_io_ok(s, 80), "the default object");
        for (int ragged = 0; ragged < 2; ++ragged) {
            const Launch512 l = route512(s, fbank_split_io_batch(ragged != 0)).run;
            CHECK(l.kernel == (ragged ? K512::kClip80Ragged : K512::kClip80) && l.waves == 8 && l.lds == Lds512::kF64PlusClipCmn && l.units_per_group == 0, "launch shape, ragged %d", ragged);
        }
        Fused512Shape t = s;
        t.cmn_power = false;
        CHECK(!fbank_split_io_ok(t, 80), "apply_cmn or use_power off");
        t = s; t.bank = Bank512::kKaldi40;
        CHECK(!fbank_split_io_ok(t, 40), "the 40-bin bank");
        t = s; t.bank = Bank512::kRuntime;
        CHECK(!fbank_split_io_ok(t, 80), "a run-time bank");
        t = s; t.fused = false;
        CHECK(!fbank_split_io_ok(t, 80), "the generic path");
        t = s; t.waves = 4;
        CHECK(!fbank_split_io_ok(t, 80), "four waves");
        t = s; t.flavor = Flavor512::kNemo;
        CHECK(!fbank_split_io_ok(t, 80), "another flavour");
    }
    static_assert(K512::kCount == static_cast<K512>(68), "the side table adds no K512");

    // ---- the dtype codes: in front of everything but the NULL object ----
    int io = -7;
    FbankSplitArgs a = fbank_split_io_codes(false, 99, 99, io);
    CHECK(a.verdict == kFbankSplitFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "fbank is NULL") && io == 0, "NULL object first");
    for (int pcm = -2; pcm <= 3; ++pcm)
        for (int out = -2; out <= 4; ++out) {
            a = fbank_split_io_codes(true, pcm, out, io);
            const bool pk = pcm == MELSPEC_PCM_F32 || pcm == MELSPEC_PCM_S16, ok = out == MELSPEC_OUT_F32 || out == MELSPEC_OUT_F16 || out == MELSPEC_OUT_BF16;
            if (pk && ok) {
                CHECK(a.verdict == kFbankSplitGo && a.status == MELSPEC_OK && io == (pcm | out << 4), "(%d, %d)", pcm, out);
            } else {
                CHECK(a.verdict == kFbankSplitFail && a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, pk ? "out_dtype" : "pcm_dtype") && io == 0,
                      "(%d, %d): %s", pcm, out, a.msg ? a.msg : "(null)");
            }
        }

    // ---- the order of the checks, against a literal table: the first row whose condition holds gives the verdict ----
    alignas(16) static char buf[64];
    const void *even = buf, *odd = buf + 1, *two = buf + 2;
    const int s16f16 = MELSPEC_PCM_S16 | MELSPEC_OUT_F16 << 4;
    // every argument bad at once, then made good one by one from the front
    struct Step { const char *what; FbankSplitVerdict verdict; int status; const char *msg; };
    const Step order[] = {
        {"apply_cmn off", kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "apply_cmn is off"},
        {"unsupported object", kFbankSplitFail, MELSPEC_ERR_UNSUPPORTED, nullptr},
        {"NULL tables", kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL"},
        {"NULL device pointer", kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "device pointer is NULL"},
        {"NULL d_means", kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "d_means is NULL"},
        {"misaligned", kFbankSplitFail, MELSPEC_ERR_INVALID_ARG, "not aligned"},
        {"go", kFbankSplitGo, MELSPEC_OK, nullptr}};
    for (int good = 0; good < 7; ++good) {
        a = fbank_split_args(good > 0, good > 1, true, 1, good > 2 ? even : nullptr, good > 2 ? even : nullptr, 1, good > 3 ? odd : nullptr, good > 3 ? odd : nullptr,
                             good > 4 ? even : nullptr, s16f16);
        if (good == 6) a = fbank_split_args(true, true, true, 1, even, even, 1, two, two, even, s16f16);
        const Step &w = order[good];
        CHECK(a.verdict == w.verdict && a.status == w.status && ((a.msg == nullptr) == (w.msg == nullptr)) && (!w.msg || std::strstr(a.msg, w.msg)), "step %d (%s): verdict %d status %d %s",
              good, w.what, a.verdict, a.status, a.msg ? a.msg : "(null)");
    }
    // n_clips == 0: OK behind the object's checks, in front of the tables; no frame at all: OK behind the tables, in front of the pointers
    CHECK(fbank_split_args(true, true, true, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, s16f16).verdict == kFbankSplitDone, "no clips: done");
    CHECK(fbank_split_args(false, true, true, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, s16f16).status == MELSPEC_ERR_INVALID_ARG, "apply_cmn before no clips");
    CHECK(fbank_split_args(true, false, true, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, s16f16).status == MELSPEC_ERR_UNSUPPORTED, "unsupported before no clips");
    CHECK(fbank_split_args(true, true, true, 3, nullptr, even, 0, nullptr, nullptr, nullptr, s16f16).verdict == kFbankSplitFail, "NULL tables before no frame");
    CHECK(fbank_split_args(true, true, true, 3, even, even, 0, nullptr, nullptr, nullptr, s16f16).verdict == kFbankSplitDone, "no frame, no d_means: done, nothing touched");
    CHECK(fbank_split_args(true, true, true, 3, even, even, 0, nullptr, nullptr, even, s16f16).verdict == kFbankSplitZero, "no frame: the mean slots are zeroed");
    CHECK(fbank_split_args(true, true, true, 3, even, even, 0, odd, odd, even, s16f16).verdict == kFbankSplitZero, "no frame: the pointers are not looked at");
    // a uniform batch has no tables
    CHECK(fbank_split_args(true, true, false, 3, nullptr, nullptr, 5, even, even, even, s16f16).verdict == kFbankSplitGo, "uniform: no tables asked for");
    CHECK(fbank_split_args(true, true, false, 3, nullptr, nullptr, 0, even, even, even, s16f16).verdict == kFbankSplitZero, "uniform: no frame");
    // alignment: natural alignment of the element type is enough, and is asked for; io = 0 is the f32 ragged split (floats both)
    for (int pcm = 0; pcm <= 1; ++pcm)
        for (int out = 0; out <= 2; ++out) {
            const int c = pcm | out << 4;
            const bool s16 = pcm == MELSPEC_PCM_S16, half = out != MELSPEC_OUT_F32;
            const struct { const void *pcm, *rows; bool bad; } cases[] = {
                {even, even, false}, {two, two, !s16 || !half}, {odd, even, true}, {even, odd, true}, {two, even, !s16}, {even, two, !half}};
            for (const auto &k : cases) {
                a = fbank_split_args(true, true, true, 1, even, even, 1, k.pcm, k.rows, even, c);
                CHECK((a.verdict == kFbankSplitFail) == k.bad && (!k.bad || (a.status == MELSPEC_ERR_INVALID_ARG && a.msg && std::strstr(a.msg, "aligned"))), "io %#x alignment", c);
            }
        }
    CHECK(fbank_split_io_pcm_bytes(MELSPEC_PCM_S16) == 2 && fbank_split_io_pcm_bytes(MELSPEC_PCM_F32) == 4 && fbank_split_io_out_bytes(MELSPEC_OUT_F32) == 4 &&
          fbank_split_io_out_bytes(MELSPEC_OUT_F16) == 2 && fbank_split_io_out_bytes(MELSPEC_OUT_BF16) == 2, "element sizes");

    if (bad) {
        std::printf("fbank_split_io_host: %d checks FAILED\n", bad);
        return 1;
    }
    std::printf("fbank_split_io_host: ok\n");
    return 0;
}
