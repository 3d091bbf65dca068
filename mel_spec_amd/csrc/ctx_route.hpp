// ctx_route.hpp -- which n_fft = 400 kernels a batch of a melspec_ctx runs on, as one pure function of the context's shape and the kind
// of batch.  The unit size a batch is planned with (ctx_frames_per_unit), the launches launch_ctx makes and the name
// melspec_plain_kernel_name reports are all read from the Route it returns.  Nothing from HIP in here: tests/cpp/route_host.cpp builds
// it with the host compiler.
#pragma once
#include "../../include/melspec_hip.h"

namespace melspec {
namespace host {

// what the decision reads of a context (ctx_shape() in host_common.hpp fills it)
struct CtxShape {
    bool fast;                 // on the fused n_fft = 400 kernels at all
    bool six;                  // the f32 six-frame kernels with nine slots (<= 80 mels)
    int six_static;            // their compile-time bank: 1 LensSix80, 2 LensSix64, 3 LensSix40, 0 run-time slot lengths
    bool six64;                // the f64 six-frame kernel
    bool six64_wide;           // ... with fifteen slots (the 128-mel bank; six is false there)
    bool six_wide32;           // the f32 six-frame kernel with fifteen slots, plain batches
    bool six_wide32_layouts;   // ... its padded / mel-major layouts too
    int lens_kind;             // the five-frame kernels' compile-time bank: 1 LensI80, 2 LensI128, 0 run-time
    int n_slots;               // mel slots of the five-frame tables
    int precision;             // MELSPEC_PRECISION_*
    bool adaptive;             // AUTO votes (melspec_set_auto_adaptive)
};

enum class BatchKind {
    kUniform,     // plain [frame][mel] rows of equal clips: the plan is arithmetic (plan_uniform)
    kRagged,      // plain rows, the plan lives in device arrays (d_unit_prefix: plan_ragged, plan_ragged_device)
    kLayout,      // padded / mel-major
    kLayoutExt,   // mel-major with the image extremes for the TGA quantiser (d_unit_ext): never votes
    kIo,          // plain, int16 PCM in and / or f16, bf16 rows out (contexts that pass io_shape_ok)
    kUnpadded,    // came in through the layout entry with nothing to pad: planned like kLayout, stored like kUniform
};

// every f32 instantiation pair (run-per-wave for plain batches, round-robin for the layouts) and every f64 instantiation
enum class F32Kernel { kNone, kSix16L80, kSix16Rt, kSix12L64, kSix12L40, kSix12x15, kWave8I80, kWave8Rt, kWave12I128, kWave12Rt, kCount };
enum class F64Kernel {
    kNone, kSix64L80, kSix64L64, kSix64L40, kSix64Rt, kSix64x15, kSix64LayoutL80, kSix64LayoutL64, kSix64LayoutL40,
    kPrecise8I80, kPrecise8Rt, kPrecise12I128, kPrecise12Rt, kCount
};
enum class F32Family { kNone, kSix16, kSix12x9, kSix12x15, kWave8, kWave12 };

constexpr F32Family family_of(F32Kernel k) {
    return k == F32Kernel::kNone ? F32Family::kNone : k <= F32Kernel::kSix16Rt ? F32Family::kSix16 : k <= F32Kernel::kSix12L40 ? F32Family::kSix12x9
         : k == F32Kernel::kSix12x15 ? F32Family::kSix12x15 : k <= F32Kernel::kWave8Rt ? F32Family::kWave8 : F32Family::kWave12;
}
// frames per unit the kernel deals in
constexpr int frames_of(F32Kernel k) { return k == F32Kernel::kNone ? 0 : k <= F32Kernel::kSix12x15 ? 6 : 5; }
constexpr int frames_of(F64Kernel k) { return k == F64Kernel::kNone ? 0 : k <= F64Kernel::kSix64LayoutL40 ? 6 : 5; }
constexpr bool is_six64(F64Kernel k) { return k >= F64Kernel::kSix64L80 && k <= F64Kernel::kSix64LayoutL40; }
constexpr bool is_six64_layout(F64Kernel k) { return k >= F64Kernel::kSix64LayoutL80 && k <= F64Kernel::kSix64LayoutL40; }

struct Route {
    int frames_per_unit;   // what the batch is planned with
    F32Kernel f32;         // the f32 launch (kNone: MELSPEC_PRECISION_F64)
    F64Kernel f64;         // the launch of MELSPEC_PRECISION_F64, or AUTO's gated second launch (kNone: no such launch)
    bool gated;            // AUTO with the vote: f64 runs behind f32 and returns at once unless that launch voted "heavy"
    int replan;            // 0: the gated launch walks the f32 launch's plan; 5 / 6: it needs the (uniform) batch planned again at that unit size
    int sync_rounds;       // RoundSync default of the first launch where the plan left it open (< 0)
    int sync_rounds64;     // ... of the gated launch
    const char *name;      // the kernel of the first launch, by its run-per-wave (plain-batch) member: melspec_plain_kernel_name's strings
};

// int16 PCM in / f16, bf16 rows out: the contexts whose plain batches run the six-frame kernels with one of the compile-time Whisper banks
// in every precision mode -- 80 mels (whisper400_six_runs_kernel + whisper400_six64_kernel<9, .>) and 128 mels
// (whisper400_six_wide_runs_kernel + whisper400_six64_kernel<15, .>)
constexpr bool io_shape_ok(const CtxShape &s) {
    return s.fast && s.six64 && ((s.six && s.six_static == 1 && !s.six64_wide) || (!s.six && s.six_wide32 && s.six64_wide));
}

inline const char *route_name(F32Kernel k, bool guarded) {
    switch (k) {
        case F32Kernel::kSix16L80: return guarded ? "melspec::whisper400_six_runs_kernel<9, LensSix80> (precision guard on)" : "melspec::whisper400_six_runs_kernel<9, LensSix80>";
        case F32Kernel::kSix16Rt: return guarded ? "melspec::whisper400_six_runs_kernel<9, LensRuntime> (precision guard on)" : "melspec::whisper400_six_runs_kernel<9, LensRuntime>";
        case F32Kernel::kSix12L64: return guarded ? "melspec::whisper400_six_wide_runs_kernel<9, LensSix64> (twelve waves; precision guard on)" : "melspec::whisper400_six_wide_runs_kernel<9, LensSix64> (twelve waves)";
        case F32Kernel::kSix12L40: return guarded ? "melspec::whisper400_six_wide_runs_kernel<9, LensSix40> (twelve waves; precision guard on)" : "melspec::whisper400_six_wide_runs_kernel<9, LensSix40> (twelve waves)";
        case F32Kernel::kSix12x15: return guarded ? "melspec::whisper400_six_wide_runs_kernel<15, LensSix128> (six frames per wave, twelve waves; precision guard on)"
                                                  : "melspec::whisper400_six_wide_runs_kernel<15, LensSix128> (six frames per wave, twelve waves)";
        case F32Kernel::kWave8I80: case F32Kernel::kWave8Rt: return guarded ? "melspec::whisper400_wave_runs_kernel<8, .> (precision guard on)" : "melspec::whisper400_wave_runs_kernel<8, .>";
        case F32Kernel::kWave12I128: case F32Kernel::kWave12Rt: return guarded ? "melspec::whisper400_wave_runs_kernel<12, .> (precision guard on)" : "melspec::whisper400_wave_runs_kernel<12, .>";
        default: return "";
    }
}
inline const char *route_name(F64Kernel k) {
    if (k == F64Kernel::kSix64x15) return "melspec::whisper400_six64_kernel<15, LensSix128> (f64 FFT, six frames per wave, three waves per SIMD, fifteen mel slots)";
    if (is_six64(k)) return "melspec::whisper400_six64_kernel<9, .> (f64 FFT, six frames per wave, three waves per SIMD)";
    if (k == F64Kernel::kPrecise8I80 || k == F64Kernel::kPrecise8Rt) return "melspec::whisper400_precise_kernel<8, ., RUNS> (f64 FFT)";
    if (k == F64Kernel::kPrecise12I128 || k == F64Kernel::kPrecise12Rt) return "melspec::whisper400_precise_kernel<12, ., RUNS> (f64 FFT)";
    return "";
}

// The route of a batch of kind `kind` on a context of shape s.  (A context off the n_fft = 400 kernels has none: launch_ctx hands its
// batches to launch_whisper512 / launch_generic, with sync_rounds 1 where the plan left it open.)
inline Route route400(const CtxShape &s, BatchKind kind) {
    Route r{1, F32Kernel::kNone, F64Kernel::kNone, false, 0, 1, 1, ""};
    if (!s.fast) return r;
    const bool f64_mode = s.precision == MELSPEC_PRECISION_F64, guarded = s.precision == MELSPEC_PRECISION_AUTO;
    const bool layout = kind == BatchKind::kLayout || kind == BatchKind::kLayoutExt;          // what the kernels store
    const bool planned_as_layout = layout || kind == BatchKind::kUnpadded;
    const bool uniform = kind != BatchKind::kRagged && kind != BatchKind::kIo;                // the host can plan it again
    // The six-frame f64 kernel serves a padded / mel-major batch only with one of the compile-time banks of up to 80 mels: its
    // run-time-lens layout instantiation keeps 141 SGPRs' worth of slot tables and reloads 13 spilled registers inside the unit loop
    // (tools/hotloop_spills.py); those banks stay on whisper400_precise_kernel's layout form.
    const bool six64_layout = s.six64 && !s.six64_wide && s.six_static != 0;

    // 1. the unit size.  AUTO plans for the f32 kernel: when the batch's vote says "heavy", the f64 kernel walks the same plan where it can.
    if (f64_mode) r.frames_per_unit = (planned_as_layout ? six64_layout : s.six64) ? 6 : 5;
    else r.frames_per_unit = (s.six || (s.six_wide32 && (!planned_as_layout || s.six_wide32_layouts))) ? 6 : 5;
    const bool six_units = r.frames_per_unit == 6;

    // 2. the f32 kernel
    if (!f64_mode) {
        if (s.six && six_units)
            r.f32 = s.six_static == 1 ? F32Kernel::kSix16L80 : s.six_static == 2 ? F32Kernel::kSix12L64 : s.six_static == 3 ? F32Kernel::kSix12L40 : F32Kernel::kSix16Rt;
        else if (s.six_wide32 && six_units) r.f32 = F32Kernel::kSix12x15;
        else if (s.n_slots <= 8) r.f32 = s.lens_kind == 1 ? F32Kernel::kWave8I80 : F32Kernel::kWave8Rt;
        else r.f32 = s.lens_kind == 2 ? F32Kernel::kWave12I128 : F32Kernel::kWave12Rt;
        // The vote: plain batches and the padded / mel-major layouts (whose sample is the head of the batch: they deal their units
        // round-robin).  Not where the mel kernel also leaves the image extremes for the TGA quantiser (the two kernels' units differ):
        // PCM -> TGA keeps the f32 kernel + recompute tail whatever the input.
        r.gated = guarded && s.adaptive && kind != BatchKind::kLayoutExt;
    }

    // 3. the f64 kernel: the whole batch in F64 mode, the gated launch in AUTO
    if (f64_mode || r.gated) {
        const F64Kernel precise = s.n_slots <= 8 ? (s.lens_kind == 1 ? F64Kernel::kPrecise8I80 : F64Kernel::kPrecise8Rt)
                                                 : (s.lens_kind == 2 ? F64Kernel::kPrecise12I128 : F64Kernel::kPrecise12Rt);
        const F64Kernel six64 = s.six64_wide ? F64Kernel::kSix64x15 : s.six_static == 1 ? F64Kernel::kSix64L80 : s.six_static == 2 ? F64Kernel::kSix64L64
                              : s.six_static == 3 ? F64Kernel::kSix64L40 : F64Kernel::kSix64Rt;
        if (layout) {
            if (six64_layout && six_units)
                r.f64 = s.six_static == 1 ? F64Kernel::kSix64LayoutL80 : s.six_static == 2 ? F64Kernel::kSix64LayoutL64 : F64Kernel::kSix64LayoutL40;
            else {
                // the layouts' other f64 kernel deals units of its own size: the same (uniform) batch planned for five frames per unit
                r.f64 = precise;
                if (six_units) r.replan = 5;
            }
        } else if (s.six64 && six_units) {
            r.f64 = six64;
        } else if (r.gated && s.six64 && s.six64_wide && uniform) {
            // 128 mels: the f32 launch walked five-frame units, the gated kernel deals six -- the same uniform batch planned again (arithmetic
            // only; a ragged batch's plan lives in device arrays made for five-frame units: those stay on the precise kernel)
            r.f64 = six64;
            r.replan = 6;
        } else {
            r.f64 = precise;          // (MODE 2 walks the f32 launch's plan whatever its unit size)
        }
    }

    // 4. RoundSync groups where the plan left them open.  Measured (profiles/r01_variants.txt): six-frame kernel, 16 waves: four waves
    // 4 apart; precise kernel, 8 waves: consecutive pairs; 5-frame kernel, two 8-wave workgroups per CU: pairs 4 apart.
    // (The groups that work are the waves of one SIMD: sixteen waves -> fours 4 apart, twelve -> threes 4 apart: the wide kernel's
    // mel-major store at 128 mels 0.532 ms with fours, 0.405-0.424 with threes, profiles/r06_wide_layouts.txt.  The 80-mel layouts on
    // twelve waves, built: 0.350 ms with threes or consecutive pairs against 0.339-0.342 on sixteen.)
    // Mel-major stores of the twelve-wave f64 kernel (tools/mm64_sync_probe.py, 1024 x 10 s): consecutive pairs 0.491 ms, none 0.493,
    // pairs four apart 0.496, fours 0.512, fours one from each SIMD (the f32 kernel's best) 0.520, workgroup barrier 0.533.
    // Twelve waves per CU (whisper400_six_wide_*: three per SIMD, 168 VGPRs): the 128-mel bank (fifteen slots) and the compile-time banks of
    // 64 and 40 mels, whose slot lengths made the sixteen-wave kernels reload spilled registers inside the unit loop (tools/isa_legs.py).
    // Measured at 1024 x 10 s, sixteen -> twelve waves (profiles/r06_wide_layouts.txt): 64 mels plain 0.381-0.386 -> 0.309-0.314 ms, mel-major
    // 0.491-0.501 -> 0.350-0.357; 40 mels plain 0.2979 -> 0.2951, mel-major 0.373 -> 0.335.  The 80-mel bank does not spill at sixteen and
    // stays there (twelve: plain 0.298 -> 0.306, mel-major 0.340 -> 0.350), as do the run-time banks.
    const bool twelve = s.six_wide32 || (s.six && (s.six_static == 2 || s.six_static == 3));
    if (f64_mode) r.sync_rounds = six_units && !layout ? (twelve ? 19 : 20) : 2;
    else r.sync_rounds = six_units ? (twelve ? 19 : 20) : 18;
    r.sync_rounds64 = layout ? 2 : r.sync_rounds;

    r.name = f64_mode ? route_name(r.f64) : route_name(r.f32, guarded);
    return r;
}

}  // namespace host
}  // namespace melspec
