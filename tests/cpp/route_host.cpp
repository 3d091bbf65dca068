// route_host.cpp -- route400 (mel_spec_amd/csrc/ctx_route.hpp) on the host: the seven context shapes of the whole-batch matrix
// (tests/test_whole_batch.py) against a literal table of kernel names and unit sizes, and the invariants of the decision over every
// combination of the shape's fields.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/route_host.cpp -o /tmp/route_host && /tmp/route_host
#include <cstdio>
#include <cstring>

#include "ctx_route.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

// N / GUARDED / F64N of tests/test_whole_batch.py
static const char *const kN[] = {
    "melspec::whisper400_six_runs_kernel<9, LensSix80>",
    "melspec::whisper400_six_wide_runs_kernel<9, LensSix64> (twelve waves)",
    "melspec::whisper400_six_wide_runs_kernel<9, LensSix40> (twelve waves)",
    "melspec::whisper400_six_runs_kernel<9, LensRuntime>",
    "melspec::whisper400_six_wide_runs_kernel<15, LensSix128> (six frames per wave, twelve waves)",
    "melspec::whisper400_wave_runs_kernel<8, .>",
    "melspec::whisper400_wave_runs_kernel<12, .>",
};
static const char *const kGuarded[] = {
    "melspec::whisper400_six_runs_kernel<9, LensSix80> (precision guard on)",
    "melspec::whisper400_six_wide_runs_kernel<9, LensSix64> (twelve waves; precision guard on)",
    "melspec::whisper400_six_wide_runs_kernel<9, LensSix40> (twelve waves; precision guard on)",
    "melspec::whisper400_six_runs_kernel<9, LensRuntime> (precision guard on)",
    "melspec::whisper400_six_wide_runs_kernel<15, LensSix128> (six frames per wave, twelve waves; precision guard on)",
    "melspec::whisper400_wave_runs_kernel<8, .> (precision guard on)",
    "melspec::whisper400_wave_runs_kernel<12, .> (precision guard on)",
};
static const char *const kSix9 = "melspec::whisper400_six64_kernel<9, .> (f64 FFT, six frames per wave, three waves per SIMD)";
static const char *const kSix15 = "melspec::whisper400_six64_kernel<15, LensSix128> (f64 FFT, six frames per wave, three waves per SIMD, fifteen mel slots)";
static const char *const kP8 = "melspec::whisper400_precise_kernel<8, ., RUNS> (f64 FFT)";
static const char *const kP12 = "melspec::whisper400_precise_kernel<12, ., RUNS> (f64 FFT)";

// what create_ctx gives 400 / 160 with the default bank of n mels in a default build (precision and adaptive are set per case);
// n_slots: ceil((n + 1) / 11) slots of the five-frame tables
struct Shape {
    int mels;
    CtxShape s;
    int fpu32;                           // FAMILIES' third column for the f32 kernel of a plain batch (AUTO, F32); the layouts plan alike
    const char *plain64, *layout64;      // F64: the name of a plain / a padded or mel-major batch ...
    int fpu_plain64, fpu_layout64;       // ... and its unit size
};
static const Shape kShapes[7] = {
    //         fast  six  static six64 wide64 wide32 w32lay lens slots
    {80,  {true, true,  1, true,  false, false, false, 1, 8,  0, true}, 6, kSix9,  kSix9, 6, 6},
    {64,  {true, true,  2, true,  false, false, false, 0, 6,  0, true}, 6, kSix9,  kSix9, 6, 6},
    {40,  {true, true,  3, true,  false, false, false, 0, 4,  0, true}, 6, kSix9,  kSix9, 6, 6},
    {60,  {true, true,  0, true,  false, false, false, 0, 6,  0, true}, 6, kSix9,  kP8,   6, 5},      // run-time lens: no six64 layout kernel
    {128, {true, false, 0, true,  true,  true,  true,  2, 12, 0, true}, 6, kSix15, kP12,  6, 5},      // fifteen slots: plain batches only in f64
    {84,  {true, false, 0, false, false, false, false, 0, 8,  0, true}, 5, kP8,    kP8,   5, 5},
    {100, {true, false, 0, false, false, false, false, 0, 10, 0, true}, 5, kP12,   kP12,  5, 5},
};
static const int kNameIndex[7] = {0, 1, 2, 3, 4, 5, 6};      // six80, six64, six40, sixrt, six128, wave8, wave12

static void literal_table() {
    for (int i = 0; i < 7; ++i)
        for (int layout = 0; layout < 2; ++layout) {
            const BatchKind kind = layout ? BatchKind::kLayout : BatchKind::kUniform;
            CtxShape s = kShapes[i].s;
            s.precision = MELSPEC_PRECISION_AUTO;
            Route r = route400(s, kind);
            CHECK(std::strcmp(r.name, kGuarded[kNameIndex[i]]) == 0 && r.frames_per_unit == kShapes[i].fpu32, "%d mels AUTO layout %d: %s, %d", kShapes[i].mels, layout, r.name, r.frames_per_unit);
            CHECK(r.gated && frames_of(r.f32) == r.frames_per_unit, "%d mels AUTO layout %d", kShapes[i].mels, layout);
            s.precision = MELSPEC_PRECISION_F32;
            r = route400(s, kind);
            CHECK(std::strcmp(r.name, kN[kNameIndex[i]]) == 0 && r.frames_per_unit == kShapes[i].fpu32, "%d mels F32 layout %d: %s, %d", kShapes[i].mels, layout, r.name, r.frames_per_unit);
            CHECK(!r.gated && r.f64 == F64Kernel::kNone, "%d mels F32 layout %d", kShapes[i].mels, layout);
            s.precision = MELSPEC_PRECISION_F64;
            r = route400(s, kind);
            CHECK(std::strcmp(r.name, layout ? kShapes[i].layout64 : kShapes[i].plain64) == 0 && r.frames_per_unit == (layout ? kShapes[i].fpu_layout64 : kShapes[i].fpu_plain64),
                  "%d mels F64 layout %d: %s, %d", kShapes[i].mels, layout, r.name, r.frames_per_unit);
            CHECK(r.f32 == F32Kernel::kNone && !r.gated, "%d mels F64 layout %d", kShapes[i].mels, layout);
        }
    // the f32 families behind FAMILIES: sixteen waves for the 80-mel and run-time banks, twelve for 64, 40 and 128 mels, the five-frame wave kernels past 80 mels
    const F32Family fam[7] = {F32Family::kSix16, F32Family::kSix12x9, F32Family::kSix12x9, F32Family::kSix16, F32Family::kSix12x15, F32Family::kWave8, F32Family::kWave12};
    const int sync[7] = {20, 19, 19, 20, 19, 18, 18};
    for (int i = 0; i < 7; ++i) {
        const Route r = route400(kShapes[i].s, BatchKind::kLayout);
        CHECK(family_of(r.f32) == fam[i] && r.sync_rounds == sync[i] && r.sync_rounds64 == 2, "%d mels: family %d, sync %d / %d", kShapes[i].mels, static_cast<int>(family_of(r.f32)), r.sync_rounds, r.sync_rounds64);
    }
    // AUTO's gated launch: the f32 plan where the f64 kernel can walk it, the batch planned again where it cannot
    CHECK(route400(kShapes[0].s, BatchKind::kLayout).f64 == F64Kernel::kSix64LayoutL80 && route400(kShapes[0].s, BatchKind::kLayout).replan == 0, "80 mels: layouts walk");
    CHECK(route400(kShapes[3].s, BatchKind::kLayout).f64 == F64Kernel::kPrecise8Rt && route400(kShapes[3].s, BatchKind::kLayout).replan == 5, "60 mels: layouts planned again at five");
    CHECK(route400(kShapes[4].s, BatchKind::kLayout).f64 == F64Kernel::kPrecise12I128 && route400(kShapes[4].s, BatchKind::kLayout).replan == 5, "128 mels: layouts planned again at five");
    CHECK(route400(kShapes[4].s, BatchKind::kRagged).f64 == F64Kernel::kSix64x15 && route400(kShapes[4].s, BatchKind::kRagged).replan == 0, "128 mels: ragged walks");
    CHECK(route400(kShapes[6].s, BatchKind::kUniform).f64 == F64Kernel::kPrecise12Rt && route400(kShapes[6].s, BatchKind::kUniform).replan == 0, "100 mels: the precise kernel walks");
    CtxShape tga = kShapes[0].s;
    CHECK(!route400(tga, BatchKind::kLayoutExt).gated && route400(tga, BatchKind::kLayoutExt).f64 == F64Kernel::kNone, "PCM -> TGA never votes");
    CHECK(io_shape_ok(kShapes[0].s) && io_shape_ok(kShapes[4].s) && !io_shape_ok(kShapes[1].s) && !io_shape_ok(kShapes[3].s) && !io_shape_ok(kShapes[5].s), "io_shape_ok: 80 and 128 mels");
}

static long invariants() {
    static const BatchKind kinds[6] = {BatchKind::kUniform, BatchKind::kRagged, BatchKind::kLayout, BatchKind::kLayoutExt, BatchKind::kIo, BatchKind::kUnpadded};
    static const int slots[4] = {6, 8, 9, 12};
    long n = 0;
    for (int bits = 0; bits < 128; ++bits)
        for (int six_static = 0; six_static < 4; ++six_static)
            for (int lens_kind = 0; lens_kind < 3; ++lens_kind)
                for (int n_slots : slots)
                    for (int precision = 0; precision < 3; ++precision)
                        for (BatchKind kind : kinds) {
                            const CtxShape s{(bits & 1) != 0, (bits & 2) != 0, six_static, (bits & 4) != 0, (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0, lens_kind, n_slots, precision, (bits & 64) != 0};
                            const Route r = route400(s, kind);
                            const bool layout = kind == BatchKind::kLayout || kind == BatchKind::kLayoutExt;
                            ++n;
#define WHERE "bits %d static %d lens %d slots %d precision %d kind %d", bits, six_static, lens_kind, n_slots, precision, static_cast<int>(kind)
                            if (!s.fast) {
                                CHECK(r.f32 == F32Kernel::kNone && r.f64 == F64Kernel::kNone && !r.gated && !r.replan && r.name, WHERE);
                                continue;
                            }
                            CHECK(r.name && r.name[0], WHERE);
                            CHECK(r.frames_per_unit == 5 || r.frames_per_unit == 6, WHERE);
                            // one of the modes' shapes: f64 alone, f32 alone, or f32 with the gated f64 behind it
                            CHECK((r.f32 == F32Kernel::kNone) == (precision == MELSPEC_PRECISION_F64), WHERE);
                            CHECK(r.gated == (precision == MELSPEC_PRECISION_AUTO && s.adaptive && kind != BatchKind::kLayoutExt), WHERE);
                            CHECK((r.f64 != F64Kernel::kNone) == (r.gated || precision == MELSPEC_PRECISION_F64), WHERE);
                            // a six-frame kernel only on six-frame units, the wave / precise kernels only on five
                            if (r.f32 != F32Kernel::kNone) CHECK(frames_of(r.f32) == r.frames_per_unit, WHERE);
                            if (precision == MELSPEC_PRECISION_F64) CHECK(frames_of(r.f64) == r.frames_per_unit && !r.replan, WHERE);
                            if (r.gated && r.replan) CHECK(frames_of(r.f64) == r.replan && r.replan != r.frames_per_unit, WHERE);
                            if (r.gated && !r.replan && (layout || is_six64(r.f64))) CHECK(frames_of(r.f64) == r.frames_per_unit, WHERE);      // (the precise kernel walks a plain plan of either size)
                            // the layout kernels that exist
                            CHECK(is_six64_layout(r.f64) == (layout && is_six64(r.f64)), WHERE);
                            if (is_six64_layout(r.f64)) CHECK(s.six64 && s.six_static != 0 && !s.six64_wide, WHERE);
                            if (layout && r.f32 == F32Kernel::kSix12x15) CHECK(s.six_wide32_layouts, WHERE);
                            // the kernels the context has tables for
                            if (family_of(r.f32) == F32Family::kSix16 || family_of(r.f32) == F32Family::kSix12x9) CHECK(s.six, WHERE);
                            if (r.f32 == F32Kernel::kSix12x15) CHECK(s.six_wide32, WHERE);
                            if (is_six64(r.f64)) CHECK(s.six64 && (r.f64 == F64Kernel::kSix64x15) == s.six64_wide, WHERE);
                            // 16-bit batches: the six-frame runs kernel and six64 in every mode, on the f32 launch's plan
                            if (kind == BatchKind::kIo && io_shape_ok(s)) {
                                CHECK(r.frames_per_unit == 6 && !r.replan, WHERE);
                                if (precision != MELSPEC_PRECISION_F64) CHECK(r.f32 == (s.six ? F32Kernel::kSix16L80 : F32Kernel::kSix12x15), WHERE);
                                if (r.f64 != F64Kernel::kNone) CHECK(r.f64 == (s.six ? F64Kernel::kSix64L80 : F64Kernel::kSix64x15), WHERE);
                            }
                            // planning again is arithmetic on a uniform batch the host can describe
                            if (r.replan) CHECK(r.gated && (kind == BatchKind::kUniform || kind == BatchKind::kLayout || kind == BatchKind::kUnpadded), WHERE);
                            // a batch without padding from the layout entry is planned like a layout
                            if (kind == BatchKind::kUnpadded) CHECK(r.frames_per_unit == route400(s, BatchKind::kLayout).frames_per_unit, WHERE);
                            if (kind == BatchKind::kRagged || kind == BatchKind::kIo) CHECK(r.frames_per_unit == route400(s, BatchKind::kUniform).frames_per_unit, WHERE);
                            if (kind == BatchKind::kLayoutExt) CHECK(r.frames_per_unit == route400(s, BatchKind::kLayout).frames_per_unit, WHERE);
#undef WHERE
                        }
    return n;
}

int main() {
    literal_table();
    const long n = invariants();
    if (bad) std::printf("FAILED (%d checks)\n", bad);
    else std::printf("route_host: ok (%ld combinations)\n", n);
    return bad ? 1 : 0;
}
