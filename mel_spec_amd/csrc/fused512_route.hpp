// fused512_route.hpp -- which kernel of the fused 512-point family (fbank512_kernels.hpp and its _io / stats siblings) a batch of the
// Kaldi fbank object, the NeMo frontend or an n_fft = 512 Whisper context runs on, as one pure function of the object's shape and the
// kind of batch.  The lists below name every instantiation the library has; fbank512.hip expands the same lists into its table of kernel
// pointers, so the two cannot drift.  The shape itself -- eight waves or four, the launch's LDS, fused or not, the bank -- comes from the
// object's tables through reach512 / shape512 below.  Nothing from HIP in here: tests/cpp/route512_host.cpp and reach512_host.cpp build it
// with the host compiler.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/melspec_hip.h"

namespace melspec {
namespace host {

// ---- every instantiation, by parameter struct ---------------------------------------------------------------------------------------
// FbankFastParams, fbank512_wave_kernel<T, WAVES, 1, kFlavor<FLAVOR>, NSLOTS, LENS, RUNS>: X(name, T, WAVES, FLAVOR, NSLOTS, LENS, RUNS).
// The f32 instantiation exists for the compile-time banks on twelve waves only, the four-wave one (tables too large for eight slices)
// with run-time slot lengths only; a RUNS kernel (name + Runs) hands each wave a contiguous run of units (frame-major plain output).
#define MS_K512_PAIR(X, name, ...) X(name, __VA_ARGS__, false) X(name##Runs, __VA_ARGS__, true)
#define MS_K512_WAVE(X)                                                     \
    MS_K512_PAIR(X, kKaldi80, double, 8, Kaldi, kFbSlots, LensKaldi80)      \
    MS_K512_PAIR(X, kKaldi40, double, 8, Kaldi, kFbSlots, LensKaldi40)      \
    MS_K512_PAIR(X, kKaldiRt, double, 8, Kaldi, kFbSlots, LensRuntime)      \
    X(kKaldiRt4, double, 4, Kaldi, kFbSlots, LensRuntime, false)            \
    X(kNemo128, double, 8, Nemo, kBlmSlots, LensSlaney128, false)           \
    X(kNemo80, double, 8, Nemo, kFbSlots, LensSlaney80, false)              \
    X(kNemoRt6, double, 8, Nemo, kFbSlots, LensRuntime, false)              \
    X(kNemoRt10, double, 8, Nemo, kBlmSlots, LensRuntime, false)            \
    X(kNemoRt6x4, double, 4, Nemo, kFbSlots, LensRuntime, false)            \
    X(kNemoRt10x4, double, 4, Nemo, kBlmSlots, LensRuntime, false)          \
    X(kNemo128F32, float, 12, Nemo, kBlmSlots, LensSlaney128, false)        \
    X(kNemo80F32, float, 12, Nemo, kFbSlots, LensSlaney80, false)           \
    MS_K512_PAIR(X, kW80, double, 8, Whisper, kFbSlots, LensSlaney80W)      \
    MS_K512_PAIR(X, kW128, double, 8, Whisper, kBlmSlots, LensSlaney128)    \
    MS_K512_PAIR(X, kWRt6, double, 8, Whisper, kFbSlots, LensRuntime)       \
    MS_K512_PAIR(X, kWRt10, double, 8, Whisper, kBlmSlots, LensRuntime)     \
    X(kWRt6x4, double, 4, Whisper, kFbSlots, LensRuntime, false)            \
    X(kWRt10x4, double, 4, Whisper, kBlmSlots, LensRuntime, false)          \
    MS_K512_PAIR(X, kW80F32, float, 12, Whisper, kFbSlots, LensSlaney80W)   \
    MS_K512_PAIR(X, kW128F32, float, 12, Whisper, kBlmSlots, LensSlaney128)
// FbankFastParams, fbank512_<FAMILY>_io_kernel<T, WAVES, NSLOTS, LENS, In, Out>: int16 PCM in and / or f16, bf16 rows out.  Five
// consecutive values per row, in the order of io_index(): X(name, In, Out, FAMILY, T, WAVES, NSLOTS, LENS)
#define MS_K512_IO5(X, name, ...)                                                                                                  \
    X(name, float, io_f16, __VA_ARGS__) X(name##_f32_bf16, float, io_bf16, __VA_ARGS__) X(name##_s16_f32, io_s16, float, __VA_ARGS__) \
    X(name##_s16_f16, io_s16, io_f16, __VA_ARGS__) X(name##_s16_bf16, io_s16, io_bf16, __VA_ARGS__)
#define MS_K512_IO(X)                                                        \
    MS_K512_IO5(X, kNemoIo128, nemo, double, 8, kBlmSlots, LensSlaney128)     \
    MS_K512_IO5(X, kNemoIo80, nemo, double, 8, kFbSlots, LensSlaney80)        \
    MS_K512_IO5(X, kNemoIo128F32, nemo, float, 12, kBlmSlots, LensSlaney128)  \
    MS_K512_IO5(X, kNemoIo80F32, nemo, float, 12, kFbSlots, LensSlaney80)     \
    MS_K512_IO5(X, kKaldiIo80, kaldi, double, 8, kFbSlots, LensKaldi80)
// FbankClipParams, fbank512_clip_kernel<NSLOTS, LENS, RAGGED> (eight f64 waves, a workgroup per clip, CMN inside): X(name, NSLOTS, LENS, RAGGED)
#define MS_K512_CLIP(X)                                  \
    X(kClip80, kFbSlots, LensKaldi80, false)             \
    X(kClip40, kFbSlots, LensKaldi40, false)             \
    X(kClipRt, kFbSlots, LensRuntime, false)             \
    X(kClip80Ragged, kFbSlots, LensKaldi80, true)        \
    X(kClip40Ragged, kFbSlots, LensKaldi40, true)        \
    X(kClipRtRagged, kFbSlots, LensRuntime, true)
// FbankStatsParams, fbank512_nemo_stats_kernel<T, WAVES, NSLOTS, LENS>: X(name, T, WAVES, NSLOTS, LENS)
#define MS_K512_STATS(X)                                         \
    X(kStats128, double, 8, kBlmSlots, LensSlaney128)            \
    X(kStats80, double, 8, kFbSlots, LensSlaney80)               \
    X(kStats128F32, float, 12, kBlmSlots, LensSlaney128)         \
    X(kStats80F32, float, 12, kFbSlots, LensSlaney80)
// W512AutoParams, w512_auto_kernel<T, WAVES, NSLOTS, LENS>: the voting f32 launch and the f64 launch gated on its verdict
#define MS_K512_AUTO(X)                                          \
    X(kAuto80Vote, float, 12, kFbSlots, LensSlaney80W)           \
    X(kAuto80Gated, double, 8, kFbSlots, LensSlaney80W)          \
    X(kAuto128Vote, float, 12, kBlmSlots, LensSlaney128)         \
    X(kAuto128Gated, double, 8, kBlmSlots, LensSlaney128)
// FbankStreamParams, fbank512_stream_kernel<T, WAVES, NSLOTS, LENS, RUNS> (fbank512_stream_kernels.hpp): the Kaldi flavour whose clips are
// the pushes of the fbank stream bank, with a "continues" flag per clip.  One per kernel a plain batch of a Kaldi object can run on, with
// that kernel's template arguments: X(name, T, WAVES, NSLOTS, LENS, RUNS)
#define MS_K512_STREAM(X)                                        \
    X(kStream80, double, 8, kFbSlots, LensKaldi80, true)         \
    X(kStream40, double, 8, kFbSlots, LensKaldi40, true)         \
    X(kStreamRt, double, 8, kFbSlots, LensRuntime, true)         \
    X(kStreamRt4, double, 4, kFbSlots, LensRuntime, false)

enum class K512 : int {
    kNone = -1,
#define MS_X(name, ...) name,
    MS_K512_WAVE(MS_X) MS_K512_IO(MS_X) MS_K512_CLIP(MS_X) MS_K512_STATS(MS_X) MS_K512_AUTO(MS_X)
    kCount,                    // the kernels of the batch calls end here; the stream bank's follow
    kStreamBase = kCount - 1,
    MS_K512_STREAM(MS_X)
#undef MS_X
    kEnd,
};
constexpr K512 operator+(K512 k, int i) { return static_cast<K512>(static_cast<int>(k) + i); }

// what a kernel is, read off the lists
struct K512Info {
    int waves;
    bool f32, runs, rt_lens;      // f32 arithmetic; a run of units per wave; run-time slot lengths
};
constexpr bool k512_same(const char *a, const char *b) { return *a == *b && (*a == 0 || k512_same(a + 1, b + 1)); }
constexpr K512Info info_of(K512 k) {
    switch (k) {
#define MS_X_WAVE(name, T, W, F, N, L, R) case K512::name: return {W, sizeof(T) == 4, R, k512_same(#L, "LensRuntime")};
#define MS_X_IO(name, In, Out, fam, T, W, N, L) case K512::name: return {W, sizeof(T) == 4, k512_same(#fam, "kaldi"), false};   // (the Kaldi _io kernel has the RUNS body)
#define MS_X_CLIP(name, N, L, R) case K512::name: return {8, false, false, k512_same(#L, "LensRuntime")};
#define MS_X_T(name, T, W, N, L) case K512::name: return {W, sizeof(T) == 4, false, false};
#define MS_X_STREAM(name, T, W, N, L, R) case K512::name: return {W, sizeof(T) == 4, R, k512_same(#L, "LensRuntime")};
        MS_K512_WAVE(MS_X_WAVE) MS_K512_IO(MS_X_IO) MS_K512_CLIP(MS_X_CLIP) MS_K512_STATS(MS_X_T) MS_K512_AUTO(MS_X_T) MS_K512_STREAM(MS_X_STREAM)
#undef MS_X_STREAM
#undef MS_X_WAVE
#undef MS_X_IO
#undef MS_X_CLIP
#undef MS_X_T
        default: return {0, false, false, false};
    }
}
// the groups, in the order of the lists
constexpr bool is_fast(K512 k) { return k >= K512::kKaldi80 && k < K512::kClip80; }
constexpr bool is_io(K512 k) { return k >= K512::kNemoIo128 && k < K512::kClip80; }
constexpr bool is_clip(K512 k) { return k >= K512::kClip80 && k < K512::kStats128; }
constexpr bool is_stats(K512 k) { return k >= K512::kStats128 && k < K512::kAuto80Vote; }
constexpr bool is_auto(K512 k) { return k >= K512::kAuto80Vote && k < K512::kCount; }
constexpr bool is_stream(K512 k) { return k >= K512::kStream80 && k < K512::kEnd; }

// ---- one launch ---------------------------------------------------------------------------------------------------------------------
// dynamic LDS of a launch: the object's f64 size, its f32 size, the f64 size plus the clip kernel's CMN block or plus RoundStats
enum class Lds512 { kF64, kF32, kF64PlusClipCmn, kF64PlusRoundStats };
struct Launch512 {
    K512 kernel;             // kNone: no such launch
    int waves;               // 64 threads each
    Lds512 lds;
    int units_per_group;     // the grid covers ceil(n_units / this) workgroups, capped per CU; 0: exactly one workgroup per CU (whole clips)
    bool lab_per_cu;         // the cap per CU is the lab knob MELSPEC_FB_GRID_PER_CU (product builds: 1); false: 1
};
constexpr Launch512 launch_of(K512 k) {
    return k == K512::kNone ? Launch512{K512::kNone, 0, Lds512::kF64, 0, false}
         : is_clip(k)       ? Launch512{k, 8, Lds512::kF64PlusClipCmn, 0, false}
         : info_of(k).f32   ? Launch512{k, info_of(k).waves, Lds512::kF32, info_of(k).waves, false}        // (an f32 stats launch keeps its partials in the staged rows)
         : is_stats(k)      ? Launch512{k, info_of(k).waves, Lds512::kF64PlusRoundStats, info_of(k).waves, false}
                            : Launch512{k, info_of(k).waves, Lds512::kF64, info_of(k).waves, !is_auto(k)};
}

// ---- the decision -------------------------------------------------------------------------------------------------------------------
enum class Flavor512 { kKaldi, kNemo, kWhisper };
// the compile-time bank whose slot lengths the object's tables have (fb_lens_match), of those its flavour has kernels for
enum class Bank512 { kRuntime, kKaldi80, kKaldi40, kSlaney80, kSlaney80W, kSlaney128 };
// what the decision reads of an object (fbank_shape / blm_shape / w512_shape in fbank512.hip fill it)
struct Fused512Shape {
    Flavor512 flavor;
    bool fused;              // on the fused 512-point kernels at all
    Bank512 bank;
    bool small_slots;        // n_slots <= kFbSlots
    int waves;               // of the f64 kernels: 8, or 4 when the tables leave no room for eight slices (reach512)
    bool f32_built;          // the f32 tables exist (Fused512F32::ok)
    int precision;           // MELSPEC_PRECISION_*
    bool adaptive;           // AUTO votes (melspec_set_auto_adaptive)
    bool auto_possible;      // the context has AUTO's statistics words
    bool cmn_power;          // Kaldi: apply_cmn on power spectra (what the workgroup-per-clip kernel computes)
};
enum class Batch512 {
    kPlain,          // frame-major rows as wide as the clips' frames, uniform or ragged
    kLayout,         // padded / mel-major (every batch of the NeMo frontend)
    kIo,             // int16 PCM in and / or f16, bf16 rows out of the mel kernel: io = pcm_dtype | out_dtype << 4, not 0
    kStats,          // the NeMo frontend's split output: rows + the partials of the row statistics
    kClipUniform,    // Kaldi + CMN, a workgroup per clip: equal clips
    kClipRagged,     // ... clips of any length, handed out by the plan's d_order
    kStream,         // Kaldi: the pushes of the fbank stream bank as a ragged plain batch, a "continues" flag per clip, rows before CMN
};
constexpr int kSyncKeep = -2;      // Route512::sync_rounds: what the plan or the caller chose stays

// ---- the shape from the tables ------------------------------------------------------------------------------------------------------
// Eight waves or four, the dynamic LDS of the f64 launch and whether the object is on the fused kernels at all: a function of the flavour
// and the bytes of the table blob, the same for the three create calls (melspec_fbank_create, melspec_blm_create, melspec_create at
// n_fft = 512) and for tests/cpp/reach512_host.cpp.  The blob grows with the length of the filters' intervals, so it is a bank of few, wide
// filters that takes four waves (1 .. 4 bins at 16 kHz), not one of many narrow ones.
constexpr size_t kLds512Limit = 160 * 1024;        // gfx950: one workgroup may use the whole LDS of a CU (kLdsLimit; fbank512.hip asserts the two agree)
constexpr size_t kSlice512Bytes = 17408;           // a wave's f64 slice, FbankLayout<double>::slice_elems() * 8 (asserted there too)
// what a flavour keeps in LDS besides the blob and the slices: the Whisper flavour 512 bytes of frame maxima per wave, the NeMo flavour
// RoundSync's sixteen counter words behind the slices
constexpr size_t lds512_per_wave(Flavor512 f) { return kSlice512Bytes + (f == Flavor512::kWhisper ? 512 : 0); }
constexpr size_t lds512_tail(Flavor512 f) { return f == Flavor512::kNemo ? 64 : 0; }
struct Reach512 {
    bool fused;              // the launch fits: the object runs on the fused 512-point kernels
    int waves;               // 8 or 4
    size_t lds_bytes;        // of a launch of `waves` f64 waves
};
constexpr Reach512 reach512_at(Flavor512 f, size_t blob_bytes, int waves) {
    const size_t lds = blob_bytes + static_cast<size_t>(waves) * lds512_per_wave(f) + lds512_tail(f);
    return Reach512{lds <= kLds512Limit, waves, lds};
}
// eight waves (two per SIMD) when everything the launch needs fits beside eight slices -- the flavour's extras included: asking with
// blob + 8 slices alone sent a NeMo bank of exactly 24 576 bytes to eight waves, 64 bytes over, and from there off the fused path --
// else four
constexpr Reach512 reach512(Flavor512 f, size_t blob_bytes) {
    return reach512_at(f, blob_bytes, 8).fused ? reach512_at(f, blob_bytes, 8) : reach512_at(f, blob_bytes, 4);
}
// do the tables' slots (a MelSlots) have exactly the compile-time slot lengths of Lens (fbank_wave.hpp)?
template <class Lens, class Slots>
bool lens_match512(const Slots &ms) {
    if (ms.n_slots != Lens::kSlots) return false;
    for (int i = 0; i < Lens::kSlots; ++i)
        if (ms.len[i] != Lens::len(i) || ms.woff[i] != Lens::woff(i)) return false;
    return true;
}
// the compile-time bank the tables have, of the two (A -> a, B -> b) the flavour has kernels for
template <class A, class B, class Slots>
Bank512 bank512(const Slots &ms, Bank512 a, Bank512 b) { return lens_match512<A>(ms) ? a : lens_match512<B>(ms) ? b : Bank512::kRuntime; }
// an object's shape as its tables give it: flavour, fused, bank, slots, waves; the precision, AUTO's and the CMN fields are the object's own
// state and start as a Kaldi object has them (f64, no f32 tables, no vote).  small_cap: kFbSlots
template <class A, class B, class Slots>
Fused512Shape shape512(Flavor512 f, const Reach512 &reach, const Slots &ms, Bank512 a, Bank512 b, int small_cap) {
    return Fused512Shape{f, reach.fused, bank512<A, B>(ms, a, b), ms.n_slots <= small_cap, reach.waves, false, MELSPEC_PRECISION_F64, false, false, false};
}

struct Route512 {
    Launch512 run;           // the batch's mel kernel
    Launch512 vote, gated;   // AUTO at n_fft = 512, a plain batch of at least w512_auto_min_units: these two instead of `run`
    int sync_rounds;         // kSyncKeep, or what BatchDesc::sync_rounds has to be for `run`
    const char *name;        // Whisper flavour: melspec_plain_kernel_name's string
};

constexpr Bank512 bank_of(const Fused512Shape &s) {
    const Bank512 b = s.bank;
    return s.flavor == Flavor512::kKaldi   ? (b == Bank512::kKaldi80 || b == Bank512::kKaldi40 ? b : Bank512::kRuntime)
         : s.flavor == Flavor512::kNemo    ? (b == Bank512::kSlaney80 || b == Bank512::kSlaney128 ? b : Bank512::kRuntime)
                                           : (b == Bank512::kSlaney80W || b == Bank512::kSlaney128 ? b : Bank512::kRuntime);
}
// the index of a (sample, row) combination among a row's five kernels; < 0: not one of them
constexpr int io_index(int io) {
    return io <= 0 || (io & 15) > MELSPEC_PCM_S16 || (io >> 4) > MELSPEC_OUT_BF16 ? -1 : (io & 15) * 3 + (io >> 4) - 1;
}
static_assert(MELSPEC_PCM_F32 == 0 && MELSPEC_PCM_S16 == 1 && MELSPEC_OUT_F32 == 0 && MELSPEC_OUT_F16 == 1 && MELSPEC_OUT_BF16 == 2, "io_index counts on the dtype codes");

// int16 PCM / f16, bf16 rows: the objects whose kernels have the instantiations -- the fused path on eight f64 waves with the compile-time
// 80-bin Kaldi bank (the frame shift is a run-time value of the kernel, the default 10 ms or not) ...
constexpr bool kaldi_io_ok(const Fused512Shape &s) { return s.flavor == Flavor512::kKaldi && s.fused && s.waves == 8 && bank_of(s) == Bank512::kKaldi80; }
// ... and with one of the compile-time Slaney banks
constexpr bool nemo_io_ok(const Fused512Shape &s) { return s.flavor == Flavor512::kNemo && s.fused && s.waves == 8 && bank_of(s) != Bank512::kRuntime; }
// the split output's kernels exist for the same contexts (the caller adds that the launch's LDS fits)
constexpr bool stats_ok(const Fused512Shape &s) { return nemo_io_ok(s); }
// can a plain batch of this n_fft = 512 context run in MELSPEC_PRECISION_AUTO's f32 / f64 pair?  (the compile-time banks, eight f64 waves)
constexpr bool w512_auto_ok(const Fused512Shape &s) {
    return s.flavor == Flavor512::kWhisper && s.fused && s.f32_built && s.waves == 8 && s.auto_possible && bank_of(s) != Bank512::kRuntime;
}
// ... when there is a batch to speak of: below two units per f32 wave of the grid (6144 units = 24 576 frames on an MI355X) a call is
// launch-bound, the pair of launches is slower than the f64 kernel alone, and the f64 kernel it is (also what keeps the streaming
// bank's hop-sized pushes on the reference's golden within 1e-6; a rule on the batch's size: still a function of the batch alone)
constexpr uint64_t w512_auto_min_units(int cus) { return 2ull * 12 * static_cast<unsigned>(cus); }
// does the object compute in f32?  (where asked for and built; the f32 kernels exist for the compile-time banks)
constexpr bool f32_mode(const Fused512Shape &s) {
    return s.flavor != Flavor512::kKaldi && s.precision == MELSPEC_PRECISION_F32 && s.f32_built && bank_of(s) != Bank512::kRuntime;
}
// the precision a plain batch of an n_fft = 512 context computes in: F32, AUTO's voting pair where the bank allows it, else f64
constexpr int w512_precision(const Fused512Shape &s) {
    return f32_mode(s) ? MELSPEC_PRECISION_F32
         : s.precision == MELSPEC_PRECISION_AUTO && s.adaptive && w512_auto_ok(s) ? MELSPEC_PRECISION_AUTO : MELSPEC_PRECISION_F64;
}
inline const char *whisper512_kernel_name(const Fused512Shape &s) {
    switch (w512_precision(s)) {
        case MELSPEC_PRECISION_F32: return "melspec::fbank512_wave_kernel<float, 12, 1, kFlavorWhisper, RUNS> (n_fft = 512, f32, three waves per SIMD)";
        case MELSPEC_PRECISION_AUTO: return "melspec::w512_auto_kernel<float, 12> (n_fft = 512, f32, precision guard + vote) + the gated melspec::w512_auto_kernel<double, 8>";
        default: return "melspec::fbank512_wave_kernel<double, 8, 1, kFlavorWhisper, RUNS> (n_fft = 512, f64)";
    }
}

// Kaldi + CMN on the workgroup-per-clip kernel: what the object and its bin count have to be (the alignment of the output is the caller's check) ...
constexpr bool clip_shape_ok(const Fused512Shape &s, int nm) {
    return s.flavor == Flavor512::kKaldi && s.fused && s.cmn_power && s.waves == 8 && nm % 4 == 0 && nm <= 89;
}
// ... equal clips: when they fill the CUs evenly enough to beat the two-kernel path's 1.29 x -- at least one clip per CU, the last pass
// over the CUs included at least 85 % full on average
constexpr bool clip_uniform_ok(uint32_t n_clips, uint32_t cus) {
    const uint32_t passes = (n_clips + cus - 1) / cus;
    return n_clips >= cus && static_cast<uint64_t>(n_clips) * 100 >= static_cast<uint64_t>(passes) * cus * 85;
}
// ... clips of any length: when the batch can keep every CU busy -- at least two clips per CU and no clip longer than half a CU's share
// (the kernel counts a clip's frames in 31 bits)
constexpr bool clip_ragged_ok(uint32_t n_clips, uint32_t cus, uint64_t longest, uint64_t total) {
    return n_clips >= 2u * cus && longest * 2 * static_cast<uint64_t>(cus) <= total && longest < (1ull << 31);
}

// The route of a batch of kind `kind` on an object of shape s; io: the (sample, row) combination of a kIo batch.  run.kernel == kNone:
// the object has no kernel for this kind of batch.
inline Route512 route512(const Fused512Shape &s, Batch512 kind, int io = 0) {
    Route512 r{launch_of(K512::kNone), launch_of(K512::kNone), launch_of(K512::kNone), kSyncKeep, ""};
    if (s.flavor == Flavor512::kWhisper) r.name = whisper512_kernel_name(s);
    if (!s.fused || (s.waves != 8 && s.waves != 4)) return r;
    const Bank512 bank = bank_of(s);
    const bool f32 = f32_mode(s), plain = kind == Batch512::kPlain, four = s.waves == 4;
    const bool small = bank == Bank512::kRuntime ? s.small_slots : bank != Bank512::kSlaney128;       // six mel slots, not ten
    K512 k = K512::kNone;
    if (s.flavor == Flavor512::kKaldi) {
        const int b = bank == Bank512::kKaldi80 ? 0 : bank == Bank512::kKaldi40 ? 1 : 2;
        if (kind == Batch512::kClipUniform || kind == Batch512::kClipRagged) {
            if (!four) k = (kind == Batch512::kClipRagged ? K512::kClip80Ragged : K512::kClip80) + b;
        } else if (kind == Batch512::kIo) {
            if (kaldi_io_ok(s) && io_index(io) >= 0) k = K512::kKaldiIo80 + io_index(io);
        } else if (kind == Batch512::kStream) {
            k = four ? K512::kStreamRt4 : K512::kStream80 + b;          // the plain batch's kernel (below) with the flag: the same rows, bit for bit
        } else if (kind != Batch512::kStats) {
            k = four ? K512::kKaldiRt4 : K512::kKaldi80 + (2 * b + (plain ? 1 : 0));
        }
    } else if (s.flavor == Flavor512::kNemo) {
        const bool wide = bank == Bank512::kSlaney128;
        if (kind == Batch512::kIo) {
            if (nemo_io_ok(s) && io_index(io) >= 0) k = (f32 ? (wide ? K512::kNemoIo128F32 : K512::kNemoIo80F32) : (wide ? K512::kNemoIo128 : K512::kNemoIo80)) + io_index(io);
        } else if (kind == Batch512::kStats) {
            if (stats_ok(s)) k = f32 ? (wide ? K512::kStats128F32 : K512::kStats80F32) : (wide ? K512::kStats128 : K512::kStats80);
        } else if (plain || kind == Batch512::kLayout) {
            k = f32 ? (wide ? K512::kNemo128F32 : K512::kNemo80F32)
              : four ? (small ? K512::kNemoRt6x4 : K512::kNemoRt10x4)
              : bank == Bank512::kRuntime ? (small ? K512::kNemoRt6 : K512::kNemoRt10) : (wide ? K512::kNemo128 : K512::kNemo80);
        }
        if (f32 && k != K512::kNone) r.sync_rounds = 0;        // StagedRows instead of RoundSync
    } else if (plain || kind == Batch512::kLayout) {
        const bool wide = bank == Bank512::kSlaney128;
        k = f32 ? (wide ? K512::kW128F32 : K512::kW80F32) + (plain ? 1 : 0)
          : four ? (small ? K512::kWRt6x4 : K512::kWRt10x4)
          : (bank == Bank512::kRuntime ? (small ? K512::kWRt6 : K512::kWRt10) : (wide ? K512::kW128 : K512::kW80)) + (plain ? 1 : 0);
        // AUTO (round 6): plain batches -- uniform and ragged -- vote like the n_fft = 400 contexts do; the layouts stay on the f64 kernel
        if (plain && w512_precision(s) == MELSPEC_PRECISION_AUTO) {
            r.vote = launch_of(wide ? K512::kAuto128Vote : K512::kAuto80Vote);
            r.gated = launch_of(wide ? K512::kAuto128Gated : K512::kAuto80Gated);
        }
    }
    r.run = launch_of(k);
    return r;
}

}  // namespace host
}  // namespace melspec
