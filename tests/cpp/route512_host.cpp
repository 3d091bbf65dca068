// route512_host.cpp -- route512 (mel_spec_amd/csrc/fused512_route.hpp) on the host: the objects the GPU suite builds against a literal
// table of kernels, waves and LDS sizes, the invariants of the decision over every combination of the shape's fields and kinds of batch,
// and the clip kernel's eligibility rules.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/route512_host.cpp -o /tmp/route512_host && /tmp/route512_host
#include <cstdio>
#include <cstring>

#include "fused512_route.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

static const char *const kNameF32 = "melspec::fbank512_wave_kernel<float, 12, 1, kFlavorWhisper, RUNS> (n_fft = 512, f32, three waves per SIMD)";
static const char *const kNameAuto = "melspec::w512_auto_kernel<float, 12> (n_fft = 512, f32, precision guard + vote) + the gated melspec::w512_auto_kernel<double, 8>";
static const char *const kNameF64 = "melspec::fbank512_wave_kernel<double, 8, 1, kFlavorWhisper, RUNS> (n_fft = 512, f64)";

constexpr int F64 = MELSPEC_PRECISION_F64, F32 = MELSPEC_PRECISION_F32, AUTO = MELSPEC_PRECISION_AUTO;
// what the create calls give: melspec_fbank_create (CMN on power spectra by default), melspec_blm_create, melspec_create at n_fft = 512
static Fused512Shape kaldi(Bank512 bank, int waves = 8) { return {Flavor512::kKaldi, true, bank, true, waves, false, F64, false, false, true}; }
static Fused512Shape nemo(Bank512 bank, bool small, int precision, int waves = 8) {
    return {Flavor512::kNemo, true, bank, small, waves, bank != Bank512::kRuntime, precision, false, false, false};
}
static Fused512Shape whisper(Bank512 bank, bool small, int precision, int waves = 8) {
    return {Flavor512::kWhisper, true, bank, small, waves, bank != Bank512::kRuntime, precision, true, true, false};
}
constexpr int io_of(int pcm, int out) { return pcm | out << 4; }

struct Row {
    const char *what;
    Fused512Shape s;
    Batch512 kind;
    int io;
    K512 kernel;
    int waves;
    Lds512 lds;
    K512 vote, gated;
    const char *name;
};
static const Row kRows[] = {
    // Kaldi fbank: the wave kernel hands each wave a run of units; many clips + CMN run on the workgroup-per-clip kernel
    {"kaldi 80 plain", kaldi(Bank512::kKaldi80), Batch512::kPlain, 0, K512::kKaldi80Runs, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 80 by clip", kaldi(Bank512::kKaldi80), Batch512::kClipUniform, 0, K512::kClip80, 8, Lds512::kF64PlusClipCmn, K512::kNone, K512::kNone, ""},
    {"kaldi 80 by clip, ragged", kaldi(Bank512::kKaldi80), Batch512::kClipRagged, 0, K512::kClip80Ragged, 8, Lds512::kF64PlusClipCmn, K512::kNone, K512::kNone, ""},
    {"kaldi 40 plain", kaldi(Bank512::kKaldi40), Batch512::kPlain, 0, K512::kKaldi40Runs, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 40 by clip", kaldi(Bank512::kKaldi40), Batch512::kClipUniform, 0, K512::kClip40, 8, Lds512::kF64PlusClipCmn, K512::kNone, K512::kNone, ""},
    {"kaldi 40 by clip, ragged", kaldi(Bank512::kKaldi40), Batch512::kClipRagged, 0, K512::kClip40Ragged, 8, Lds512::kF64PlusClipCmn, K512::kNone, K512::kNone, ""},
    {"kaldi run-time plain", kaldi(Bank512::kRuntime), Batch512::kPlain, 0, K512::kKaldiRtRuns, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi run-time by clip", kaldi(Bank512::kRuntime), Batch512::kClipUniform, 0, K512::kClipRt, 8, Lds512::kF64PlusClipCmn, K512::kNone, K512::kNone, ""},
    {"kaldi run-time by clip, ragged", kaldi(Bank512::kRuntime), Batch512::kClipRagged, 0, K512::kClipRtRagged, 8, Lds512::kF64PlusClipCmn, K512::kNone, K512::kNone, ""},
    {"kaldi 80 (f32, f16)", kaldi(Bank512::kKaldi80), Batch512::kIo, io_of(MELSPEC_PCM_F32, MELSPEC_OUT_F16), K512::kKaldiIo80, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 80 (f32, bf16)", kaldi(Bank512::kKaldi80), Batch512::kIo, io_of(MELSPEC_PCM_F32, MELSPEC_OUT_BF16), K512::kKaldiIo80_f32_bf16, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 80 (s16, f32)", kaldi(Bank512::kKaldi80), Batch512::kIo, io_of(MELSPEC_PCM_S16, MELSPEC_OUT_F32), K512::kKaldiIo80_s16_f32, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 80 (s16, f16)", kaldi(Bank512::kKaldi80), Batch512::kIo, io_of(MELSPEC_PCM_S16, MELSPEC_OUT_F16), K512::kKaldiIo80_s16_f16, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 80 (s16, bf16)", kaldi(Bank512::kKaldi80), Batch512::kIo, io_of(MELSPEC_PCM_S16, MELSPEC_OUT_BF16), K512::kKaldiIo80_s16_bf16, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"kaldi 40 has no 16-bit kernel", kaldi(Bank512::kKaldi40), Batch512::kIo, io_of(MELSPEC_PCM_S16, MELSPEC_OUT_F16), K512::kNone, 0, Lds512::kF64, K512::kNone, K512::kNone, ""},
    // NeMo frontend: feature-major rows, never a run per wave
    {"nemo 80 f64 raw", nemo(Bank512::kSlaney80, true, F64), Batch512::kLayout, 0, K512::kNemo80, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo 80 f64 (s16, f16)", nemo(Bank512::kSlaney80, true, F64), Batch512::kIo, io_of(1, 1), K512::kNemoIo80_s16_f16, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo 80 f64 stats", nemo(Bank512::kSlaney80, true, AUTO), Batch512::kStats, 0, K512::kStats80, 8, Lds512::kF64PlusRoundStats, K512::kNone, K512::kNone, ""},
    {"nemo 80 f32 raw", nemo(Bank512::kSlaney80, true, F32), Batch512::kLayout, 0, K512::kNemo80F32, 12, Lds512::kF32, K512::kNone, K512::kNone, ""},
    {"nemo 80 f32 (f32, bf16)", nemo(Bank512::kSlaney80, true, F32), Batch512::kIo, io_of(0, 2), K512::kNemoIo80F32_f32_bf16, 12, Lds512::kF32, K512::kNone, K512::kNone, ""},
    {"nemo 80 f32 stats", nemo(Bank512::kSlaney80, true, F32), Batch512::kStats, 0, K512::kStats80F32, 12, Lds512::kF32, K512::kNone, K512::kNone, ""},
    {"nemo 128 f64 raw", nemo(Bank512::kSlaney128, false, AUTO), Batch512::kLayout, 0, K512::kNemo128, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo 128 f64 (s16, f32)", nemo(Bank512::kSlaney128, false, F64), Batch512::kIo, io_of(1, 0), K512::kNemoIo128_s16_f32, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo 128 f64 stats", nemo(Bank512::kSlaney128, false, F64), Batch512::kStats, 0, K512::kStats128, 8, Lds512::kF64PlusRoundStats, K512::kNone, K512::kNone, ""},
    {"nemo 128 f32 raw", nemo(Bank512::kSlaney128, false, F32), Batch512::kLayout, 0, K512::kNemo128F32, 12, Lds512::kF32, K512::kNone, K512::kNone, ""},
    {"nemo 128 f32 (f32, f16)", nemo(Bank512::kSlaney128, false, F32), Batch512::kIo, io_of(0, 1), K512::kNemoIo128F32, 12, Lds512::kF32, K512::kNone, K512::kNone, ""},
    {"nemo 128 f32 stats", nemo(Bank512::kSlaney128, false, F32), Batch512::kStats, 0, K512::kStats128F32, 12, Lds512::kF32, K512::kNone, K512::kNone, ""},
    {"nemo run-time, <= kFbSlots slots", nemo(Bank512::kRuntime, true, F32), Batch512::kLayout, 0, K512::kNemoRt6, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo run-time, > kFbSlots slots", nemo(Bank512::kRuntime, false, AUTO), Batch512::kLayout, 0, K512::kNemoRt10, 8, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo run-time has no stats kernel", nemo(Bank512::kRuntime, false, AUTO), Batch512::kStats, 0, K512::kNone, 0, Lds512::kF64, K512::kNone, K512::kNone, ""},
    // Whisper at n_fft = 512: plain batches run per wave and vote in AUTO, the layouts deal round-robin and stay on the f64 kernel
    {"w512 80 f32 plain", whisper(Bank512::kSlaney80W, true, F32), Batch512::kPlain, 0, K512::kW80F32Runs, 12, Lds512::kF32, K512::kNone, K512::kNone, kNameF32},
    {"w512 80 f32 layout", whisper(Bank512::kSlaney80W, true, F32), Batch512::kLayout, 0, K512::kW80F32, 12, Lds512::kF32, K512::kNone, K512::kNone, kNameF32},
    {"w512 80 f64 plain", whisper(Bank512::kSlaney80W, true, F64), Batch512::kPlain, 0, K512::kW80Runs, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 80 f64 layout", whisper(Bank512::kSlaney80W, true, F64), Batch512::kLayout, 0, K512::kW80, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 80 auto plain", whisper(Bank512::kSlaney80W, true, AUTO), Batch512::kPlain, 0, K512::kW80Runs, 8, Lds512::kF64, K512::kAuto80Vote, K512::kAuto80Gated, kNameAuto},
    {"w512 80 auto layout", whisper(Bank512::kSlaney80W, true, AUTO), Batch512::kLayout, 0, K512::kW80, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameAuto},
    {"w512 128 f32 plain", whisper(Bank512::kSlaney128, false, F32), Batch512::kPlain, 0, K512::kW128F32Runs, 12, Lds512::kF32, K512::kNone, K512::kNone, kNameF32},
    {"w512 128 f32 layout", whisper(Bank512::kSlaney128, false, F32), Batch512::kLayout, 0, K512::kW128F32, 12, Lds512::kF32, K512::kNone, K512::kNone, kNameF32},
    {"w512 128 f64 plain", whisper(Bank512::kSlaney128, false, F64), Batch512::kPlain, 0, K512::kW128Runs, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 128 f64 layout", whisper(Bank512::kSlaney128, false, F64), Batch512::kLayout, 0, K512::kW128, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 128 auto plain", whisper(Bank512::kSlaney128, false, AUTO), Batch512::kPlain, 0, K512::kW128Runs, 8, Lds512::kF64, K512::kAuto128Vote, K512::kAuto128Gated, kNameAuto},
    {"w512 128 auto layout", whisper(Bank512::kSlaney128, false, AUTO), Batch512::kLayout, 0, K512::kW128, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameAuto},
    {"w512 run-time plain", whisper(Bank512::kRuntime, true, AUTO), Batch512::kPlain, 0, K512::kWRt6Runs, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 run-time layout", whisper(Bank512::kRuntime, true, F32), Batch512::kLayout, 0, K512::kWRt6, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 run-time, > kFbSlots slots", whisper(Bank512::kRuntime, false, F64), Batch512::kPlain, 0, K512::kWRt10Runs, 8, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    // tables that leave no room for eight slices: four waves, run-time slot lengths whatever the bank
    {"kaldi 80 on four waves", kaldi(Bank512::kKaldi80, 4), Batch512::kPlain, 0, K512::kKaldiRt4, 4, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo 128 on four waves", nemo(Bank512::kSlaney128, false, F64, 4), Batch512::kLayout, 0, K512::kNemoRt10x4, 4, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"nemo run-time on four waves", nemo(Bank512::kRuntime, true, F64, 4), Batch512::kLayout, 0, K512::kNemoRt6x4, 4, Lds512::kF64, K512::kNone, K512::kNone, ""},
    {"w512 run-time on four waves", whisper(Bank512::kRuntime, true, AUTO, 4), Batch512::kPlain, 0, K512::kWRt6x4, 4, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
    {"w512 128 on four waves", whisper(Bank512::kRuntime, false, F64, 4), Batch512::kLayout, 0, K512::kWRt10x4, 4, Lds512::kF64, K512::kNone, K512::kNone, kNameF64},
};

static void literal_table() {
    for (const Row &w : kRows) {
        const Route512 r = route512(w.s, w.kind, w.io);
        CHECK(r.run.kernel == w.kernel && r.run.waves == w.waves && r.run.lds == w.lds, "%s: kernel %d, %d waves, lds %d", w.what, static_cast<int>(r.run.kernel), r.run.waves, static_cast<int>(r.run.lds));
        CHECK(r.vote.kernel == w.vote && r.gated.kernel == w.gated, "%s: pair %d, %d", w.what, static_cast<int>(r.vote.kernel), static_cast<int>(r.gated.kernel));
        CHECK(std::strcmp(r.name, w.name) == 0, "%s: name %s", w.what, r.name);
        // the grid: a workgroup per CU for whole clips, else one per `waves` units; the lab knob only on the f64 wave kernels
        if (w.kernel != K512::kNone) {
            CHECK(r.run.units_per_group == (is_clip(w.kernel) ? 0 : w.waves), "%s: %d units per workgroup", w.what, r.run.units_per_group);
            CHECK(r.run.lab_per_cu == (is_fast(w.kernel) && w.lds == Lds512::kF64), "%s: per-CU knob %d", w.what, r.run.lab_per_cu);
        }
        // StagedRows instead of RoundSync: the f32 NeMo kernels, and only they
        CHECK(r.sync_rounds == (w.s.flavor == Flavor512::kNemo && w.lds == Lds512::kF32 ? 0 : kSyncKeep), "%s: sync_rounds %d", w.what, r.sync_rounds);
    }
    // AUTO's pair: twelve f32 waves on the f32 tables, eight f64 waves, neither with the lab knob
    const Route512 a = route512(whisper(Bank512::kSlaney80W, true, AUTO), Batch512::kPlain);
    CHECK(a.vote.waves == 12 && a.vote.lds == Lds512::kF32 && a.vote.units_per_group == 12 && !a.vote.lab_per_cu, "the voting launch");
    CHECK(a.gated.waves == 8 && a.gated.lds == Lds512::kF64 && a.gated.units_per_group == 8 && !a.gated.lab_per_cu, "the gated launch");
    CHECK(w512_auto_min_units(256) == 6144, "two units per f32 wave of the grid");
    Fused512Shape off = whisper(Bank512::kSlaney80W, true, AUTO);
    off.adaptive = false;
    CHECK(route512(off, Batch512::kPlain).vote.kernel == K512::kNone && std::strcmp(route512(off, Batch512::kPlain).name, kNameF64) == 0, "AUTO without the vote is f64 at 512");
    // an object on the generic path has no route
    Fused512Shape generic = kaldi(Bank512::kKaldi80);
    generic.fused = false;
    CHECK(route512(generic, Batch512::kPlain).run.kernel == K512::kNone && !kaldi_io_ok(generic) && !clip_shape_ok(generic, 80), "melspec_fbank_use_generic");
    CHECK(static_cast<int>(K512::kCount) == 68, "%d kernels", static_cast<int>(K512::kCount));
}

static bool kernel_of_flavor(K512 k, Flavor512 f) {
    if (k == K512::kNone) return true;
    if (f == Flavor512::kKaldi) return (k >= K512::kKaldi80 && k <= K512::kKaldiRt4) || (k >= K512::kKaldiIo80 && k <= K512::kKaldiIo80_s16_bf16) || is_clip(k);
    if (f == Flavor512::kNemo) return (k >= K512::kNemo128 && k <= K512::kNemo80F32) || (k >= K512::kNemoIo128 && k < K512::kKaldiIo80) || is_stats(k);
    return (k >= K512::kW80 && k <= K512::kW128F32Runs) || is_auto(k);
}

static long invariants() {
    static const Batch512 kinds[6] = {Batch512::kPlain, Batch512::kLayout, Batch512::kIo, Batch512::kStats, Batch512::kClipUniform, Batch512::kClipRagged};
    static const int ios[9] = {0, io_of(1, 0), io_of(0, 1), io_of(1, 1), io_of(0, 2), io_of(1, 2), io_of(2, 0), io_of(0, 3), -1};
    long n = 0;
    for (int flavor = 0; flavor < 3; ++flavor)
        for (int bank = 0; bank < 6; ++bank)
            for (int bits = 0; bits < 128; ++bits)
                for (int precision = 0; precision < 3; ++precision)
                    for (Batch512 kind : kinds)
                        for (int io : ios) {
                            const Fused512Shape s{static_cast<Flavor512>(flavor), (bits & 1) != 0, static_cast<Bank512>(bank), (bits & 2) != 0, (bits & 4) ? 8 : 4, (bits & 8) != 0,
                                                  precision, (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0};
                            const Route512 r = route512(s, kind, io);
                            const K512 k = r.run.kernel;
                            const K512Info ki = info_of(k);
                            const bool static_bank = bank_of(s) != Bank512::kRuntime;
                            ++n;
#define WHERE "flavor %d bank %d bits %d precision %d kind %d io %d -> %d", flavor, bank, bits, precision, static_cast<int>(kind), io, static_cast<int>(k)
                            // the name is one of the three literals (Whisper) or empty (the two objects have none)
                            if (s.flavor == Flavor512::kWhisper) CHECK(r.name == whisper512_kernel_name(s) && (!std::strcmp(r.name, kNameF32) || !std::strcmp(r.name, kNameAuto) || !std::strcmp(r.name, kNameF64)), WHERE);
                            else CHECK(r.name[0] == 0, WHERE);
                            if (!s.fused) {
                                CHECK(k == K512::kNone && r.vote.kernel == K512::kNone && r.gated.kernel == K512::kNone, WHERE);
                                continue;
                            }
                            // the launch is the kernel's: its waves, its group's LDS
                            CHECK(kernel_of_flavor(k, s.flavor) && kernel_of_flavor(r.vote.kernel, s.flavor) && kernel_of_flavor(r.gated.kernel, s.flavor), WHERE);
                            CHECK(k == K512::kNone || (r.run.waves == ki.waves && (r.run.lds == Lds512::kF32) == ki.f32 && (r.run.lds == Lds512::kF64PlusClipCmn) == is_clip(k) &&
                                                       (r.run.lds == Lds512::kF64PlusRoundStats) == (is_stats(k) && !ki.f32)), WHERE);
                            // plain and layout batches of a fused object always have a kernel
                            if (kind == Batch512::kPlain || kind == Batch512::kLayout) CHECK(k != K512::kNone && is_fast(k) && !is_io(k), WHERE);
                            // an f32 kernel only with a compile-time bank and built f32 tables, in F32 mode
                            if (ki.f32) CHECK(static_bank && s.f32_built && s.precision == MELSPEC_PRECISION_F32 && s.flavor != Flavor512::kKaldi && ki.waves == 12, WHERE);
                            // the four-wave kernel only for f64 with run-time lens, on objects whose tables ask for it; eight otherwise
                            if (ki.waves == 4) CHECK(!ki.f32 && ki.rt_lens && s.waves == 4 && !is_io(k) && !is_clip(k) && !is_stats(k), WHERE);
                            if (ki.waves == 8) CHECK(s.waves == 8, WHERE);
                            // run-time slot lengths only without a compile-time bank (or on four waves), a compile-time bank's kernel only with it
                            if (k != K512::kNone && ki.waves != 4) CHECK(ki.rt_lens == !static_bank, WHERE);
                            // a run per wave only for frame-major plain rows, never for the NeMo frontend
                            if (ki.runs) CHECK(s.flavor != Flavor512::kNemo && (kind == Batch512::kPlain || kind == Batch512::kIo) && (ki.waves == 8 || ki.waves == 12), WHERE);
                            if (kind == Batch512::kPlain && s.flavor != Flavor512::kNemo && ki.waves != 4) CHECK(ki.runs, WHERE);
                            // 16-bit and stats kernels only where the matching predicate holds, and there always
                            const bool io_ok = (s.flavor == Flavor512::kKaldi ? kaldi_io_ok(s) : nemo_io_ok(s)) && io_index(io) >= 0;
                            CHECK(is_io(k) == (kind == Batch512::kIo && io_ok), WHERE);
                            if (is_io(k)) CHECK(static_cast<int>(k) % 5 == (static_cast<int>(K512::kNemoIo128) + io_index(io)) % 5, WHERE);
                            CHECK(is_stats(k) == (kind == Batch512::kStats && stats_ok(s)), WHERE);
                            CHECK(is_clip(k) == ((kind == Batch512::kClipUniform || kind == Batch512::kClipRagged) && s.flavor == Flavor512::kKaldi && s.waves == 8), WHERE);
                            if (clip_shape_ok(s, 80)) CHECK(is_clip(route512(s, Batch512::kClipUniform).run.kernel) && is_clip(route512(s, Batch512::kClipRagged).run.kernel), WHERE);
                            // AUTO's pair only where w512_auto_ok holds, the mode is AUTO with the vote and the batch is plain
                            const bool pair = kind == Batch512::kPlain && w512_auto_ok(s) && s.precision == MELSPEC_PRECISION_AUTO && s.adaptive;
                            CHECK((r.vote.kernel != K512::kNone) == pair && (r.gated.kernel != K512::kNone) == pair, WHERE);
                            if (pair) CHECK(is_auto(r.vote.kernel) && info_of(r.vote.kernel).f32 && r.gated.kernel == r.vote.kernel + 1 && !info_of(r.gated.kernel).f32 && !ki.f32 && ki.runs, WHERE);
                            CHECK((w512_precision(s) == MELSPEC_PRECISION_AUTO) == (w512_auto_ok(s) && s.precision == MELSPEC_PRECISION_AUTO && s.adaptive), WHERE);
                            // RoundSync is overridden for the f32 NeMo kernels only
                            CHECK(r.sync_rounds == (s.flavor == Flavor512::kNemo && ki.f32 ? 0 : kSyncKeep), WHERE);
#undef WHERE
                        }
    return n;
}

static void clip_rules() {
    const uint32_t cus = 256;
    // equal clips: at least one per CU, the passes over the CUs at least 85 % full
    CHECK(!clip_uniform_ok(255, cus), "255 clips");
    CHECK(clip_uniform_ok(256, cus), "256 clips");
    CHECK(!clip_uniform_ok(257, cus), "257 clips: two passes, 25 700 < 43 520");
    CHECK(!clip_uniform_ok(435, cus), "435 clips: 43 500 < 43 520");
    CHECK(clip_uniform_ok(436, cus), "436 clips: 43 600 >= 43 520");
    CHECK(clip_uniform_ok(3 * cus, cus) && clip_uniform_ok(5 * cus - cus / 8, cus) && !clip_uniform_ok(4 * cus + 1, cus), "the tiny-clips matrix");
    // clips of any length: at least two per CU, none longer than half a CU's share, 31-bit frame counts
    CHECK(!clip_ragged_ok(511, cus, 100, 511 * 100), "511 clips");
    CHECK(clip_ragged_ok(512, cus, 100, 512 * 100), "512 equal clips");
    CHECK(!clip_ragged_ok(512, cus, 101, 511 * 100 + 101), "one clip just past total / 512");
    CHECK(clip_ragged_ok(5 * cus, cus, 36, 5ull * cus * 20), "many tiny clips");
    CHECK(!clip_ragged_ok(512, cus, 1ull << 31, 512ull << 31), "longest = 2^31");
    CHECK(clip_ragged_ok(512, cus, (1ull << 31) - 1, 512 * ((1ull << 31) - 1)), "longest = 2^31 - 1");
    // either: the bin count (rows of whole 16-byte granules, six mel slots), CMN on power spectra, eight waves
    const Fused512Shape k = kaldi(Bank512::kKaldi80);
    CHECK(clip_shape_ok(k, 88) && clip_shape_ok(k, 80) && clip_shape_ok(k, 40) && clip_shape_ok(k, 24), "n_mels = 88");
    CHECK(!clip_shape_ok(k, 89), "n_mels = 89: 89 %% 4 != 0");
    CHECK(!clip_shape_ok(k, 92) && !clip_shape_ok(k, 82), "n_mels = 92");
    Fused512Shape no_cmn = k;
    no_cmn.cmn_power = false;
    CHECK(!clip_shape_ok(no_cmn, 80) && !clip_shape_ok(kaldi(Bank512::kKaldi80, 4), 80) && !clip_shape_ok(nemo(Bank512::kSlaney80, true, F64), 80), "CMN, eight waves, Kaldi");
}

int main() {
    literal_table();
    const long n = invariants();
    clip_rules();
    if (bad) std::printf("FAILED (%d checks)\n", bad);
    else std::printf("route512_host: ok (%ld combinations)\n", n);
    return bad ? 1 : 0;
}
