// fbank512.hip -- the fused 512-point family (fbank512_kernels.hpp) and the two objects of the C ABI that live on it: the Kaldi fbank
// context (melspec_fbank_*, src/fbank.rs:94-313) and the NeMo / Parakeet frontend (melspec_blm_*, src/mel.rs:239-396); Whisper at n_fft = 512
// reaches the same kernels through launch_whisper512.
#include "host_common.hpp"
#include "fbank512_io_kernels.hpp"
#include "fbank512_kaldi_io_kernels.hpp"
#include "fbank512_kaldi_split_io_kernels.hpp"
#include "fbank512_stats_kernels.hpp"
#include "fbank512_stats_ragged_kernels.hpp"
#include "fbank512_stats_io_kernels.hpp"
#include "fbank512_stream_kernels.hpp"
#include "fbank512_nemo_stream_kernels.hpp"
#include "stream_banks_io_kernels.hpp"
#include "blm_stats_plan.hpp"
#include "blm_split_io_plan.hpp"
#include "fbank_split_io_plan.hpp"
#include "blm_stream_plan.hpp"
#include "fbank_stream_plan.hpp"
#include "stat_bank.hpp"

namespace melspec {
// emitted by fbank512_io.hip / fbank512_kaldi_io.hip: the NeMo frontend and the Kaldi fbank with int16 PCM in and / or f16, bf16 rows out
#define MS_IO_EXTERN(name, In, Out, fam, T, W, N, L) extern template __global__ void fbank512_##fam##_io_kernel<T, W, N, L, In, Out>(const FbankFastParams);
MS_K512_IO(MS_IO_EXTERN)
#undef MS_IO_EXTERN
extern template __global__ void blm_normalize_io_kernel<io_f16>(const BlmNormIoParams);
extern template __global__ void blm_normalize_io_kernel<io_bf16>(const BlmNormIoParams);
extern template __global__ void blm_normalize_ragged_io_kernel<io_f16>(const BlmNormRaggedIoParams);
extern template __global__ void blm_normalize_ragged_io_kernel<io_bf16>(const BlmNormRaggedIoParams);
extern template __global__ void cmn_io_kernel<io_f16>(const CmnIoParams);
extern template __global__ void cmn_io_kernel<io_bf16>(const CmnIoParams);
// emitted by fbank512_stats.hip: the NeMo frontend's split output (rows + the partials of the row statistics)
#define MS_STATS_EXTERN(name, T, W, N, L) extern template __global__ void fbank512_nemo_stats_kernel<T, W, N, L>(const FbankStatsParams);
MS_K512_STATS(MS_STATS_EXTERN)
#undef MS_STATS_EXTERN
// emitted by fbank512_stats_ragged.hip: the ragged form of the split output, one kernel per kernel of the list above
#define MS_STATS_RAGGED_EXTERN(name, T, W, N, L) extern template __global__ void fbank512_nemo_stats_ragged_kernel<T, W, N, L>(const FbankStatsRaggedParams);
MS_K512_STATS(MS_STATS_RAGGED_EXTERN)
#undef MS_STATS_RAGGED_EXTERN
// emitted by fbank512_stream.hip: the Kaldi fbank's stream bank (the plain kernels with a "continues" flag per clip)
#define MS_STREAM_EXTERN(name, T, W, N, L, R) extern template __global__ void fbank512_stream_kernel<T, W, N, L, R>(const FbankStreamParams);
MS_K512_STREAM(MS_STREAM_EXTERN)
#undef MS_STREAM_EXTERN
// emitted by fbank512_nemo_stream.hip: the NeMo frontend's stream bank (the batch kernels with a window origin per clip)
#define MS_NEMO_STREAM_EXTERN(name, T, W, N, L) extern template __global__ void fbank512_nemo_stream_kernel<T, W, N, L>(const FbankNemoStreamParams);
MS_K512_NEMO_STREAM(MS_NEMO_STREAM_EXTERN)
#undef MS_NEMO_STREAM_EXTERN
}  // namespace melspec

namespace {
// ---- the kernel behind every K512 (the lists of fused512_route.hpp), by parameter struct; one launcher for them all ----------------------
// MELSPEC_PRECISION_F32: twelve waves = three per SIMD (158-168 VGPRs without spills; at sixteen waves the 128-VGPR budget spills 24-38
// registers inside the unit loop and the kernel is slower than the f64 one, profiles/r05_fb512_twelve_waves.txt)
#define MS_WAVE(name, T, W, F, N, L, R)                                                                                     \
    static_assert(sizeof(T) == 8 ? (W == 8 || (W == 4 && !L::kStatic)) : (W == kFused512F32Waves && L::kStatic),            \
                  "the f32 instantiation exists for the compile-time banks, the four-wave one for run-time slot lengths");
MS_K512_WAVE(MS_WAVE)
#undef MS_WAVE
#define MS_WAVE(name, T, W, F, N, L, R) &fbank512_wave_kernel<T, W, 1, kFlavor##F, N, L, R>,
#define MS_IO(name, In, Out, fam, T, W, N, L) &fbank512_##fam##_io_kernel<T, W, N, L, In, Out>,
#define MS_CLIP(name, N, L, R) &fbank512_clip_kernel<N, L, R>,
#define MS_STATS(name, T, W, N, L) &fbank512_nemo_stats_kernel<T, W, N, L>,
#define MS_STATS_RAGGED(name, T, W, N, L) &fbank512_nemo_stats_ragged_kernel<T, W, N, L>,
#define MS_AUTO(name, T, W, N, L) &w512_auto_kernel<T, W, N, L>,
#define MS_STREAM(name, T, W, N, L, R) &fbank512_stream_kernel<T, W, N, L, R>,
void (*const kFastKernels[])(const FbankFastParams) = {MS_K512_WAVE(MS_WAVE) MS_K512_IO(MS_IO)};
void (*const kClipKernels[])(const FbankClipParams) = {MS_K512_CLIP(MS_CLIP)};
void (*const kStatsKernels[])(const FbankStatsParams) = {MS_K512_STATS(MS_STATS)};
void (*const kStatsRaggedKernels[])(const FbankStatsRaggedParams) = {MS_K512_STATS(MS_STATS_RAGGED)};       // keyed by the uniform call's kernel: same launch shape, same LDS
void (*const kAutoKernels[])(const W512AutoParams) = {MS_K512_AUTO(MS_AUTO)};
void (*const kStreamKernels[])(const FbankStreamParams) = {MS_K512_STREAM(MS_STREAM)};
#undef MS_WAVE
#undef MS_IO
#undef MS_CLIP
#undef MS_STATS
#undef MS_STATS_RAGGED
#undef MS_AUTO
#undef MS_STREAM
constexpr int idx(K512 k) { return static_cast<int>(k); }
static_assert(sizeof(kFastKernels) / sizeof(kFastKernels[0]) == idx(K512::kClip80) && sizeof(kClipKernels) / sizeof(kClipKernels[0]) == idx(K512::kStats128) - idx(K512::kClip80) &&
              sizeof(kStatsKernels) / sizeof(kStatsKernels[0]) == idx(K512::kAuto80Vote) - idx(K512::kStats128) &&
              sizeof(kAutoKernels) / sizeof(kAutoKernels[0]) == idx(K512::kCount) - idx(K512::kAuto80Vote) &&
              sizeof(kStreamKernels) / sizeof(kStreamKernels[0]) == idx(K512::kEnd) - idx(K512::kStream80) && idx(K512::kStream80) == idx(K512::kCount),
              "one kernel per K512, in the order of the lists");
static_assert(kFused512F32Waves == 12, "fused512_route.hpp spells the f32 kernels' waves out");

inline auto kernel512(K512 k, const FbankFastParams &) { return is_fast(k) ? kFastKernels[idx(k)] : nullptr; }
inline auto kernel512(K512 k, const FbankClipParams &) { return is_clip(k) ? kClipKernels[idx(k) - idx(K512::kClip80)] : nullptr; }
inline auto kernel512(K512 k, const FbankStatsParams &) { return is_stats(k) ? kStatsKernels[idx(k) - idx(K512::kStats128)] : nullptr; }
inline auto kernel512(K512 k, const FbankStatsRaggedParams &) { return is_stats(k) ? kStatsRaggedKernels[idx(k) - idx(K512::kStats128)] : nullptr; }
inline auto kernel512(K512 k, const W512AutoParams &) { return is_auto(k) ? kAutoKernels[idx(k) - idx(K512::kAuto80Vote)] : nullptr; }
inline auto kernel512(K512 k, const FbankStreamParams &) { return is_stream(k) ? kStreamKernels[idx(k) - idx(K512::kStream80)] : nullptr; }
// the NeMo stream bank's kernels have a table of their own, keyed by the kernel a batch of the object runs on: same launch shape, same LDS
inline auto kernel512(K512 k, const FbankNemoStreamParams &) { return nemo_stream_kernel(k); }
inline const BatchDesc &batch_of(const FbankFastParams &p) { return p.b; }
template <class P> const BatchDesc &batch_of(const P &q) { return q.f.b; }

// an object's dynamic LDS: of its f64 kernels, of its f32 kernels (0: none), and the bin count RoundStats is sized by
struct Lds512Sizes {
    size_t f64, f32;
    int n_mels;
};
size_t lds512(Lds512 which, const Lds512Sizes &z) {
    switch (which) {
        case Lds512::kF32: return z.f32;
        case Lds512::kF64PlusClipCmn: return z.f64 + sizeof(ClipCmnShared<8>);
        case Lds512::kF64PlusRoundStats: return z.f64 + RoundStats<8>::bytes(z.n_mels);
        default: return z.f64;
    }
}
unsigned grid512(const Launch512 &l, uint64_t n_units, int cus) {
    static const int per_cu = lab_int("MELSPEC_FB_GRID_PER_CU", 1, 1, 4096);   // one workgroup is resident per CU; measured best
    if (l.units_per_group == 0) return static_cast<unsigned>(cus);
    return grid_for_xcd((n_units + l.units_per_group - 1) / l.units_per_group, cus, l.lab_per_cu ? per_cu : 1);
}
const char *attr_name(K512 k) {
    return is_clip(k) ? "hipFuncSetAttribute(fbank512_clip_kernel)" : is_stats(k) ? "hipFuncSetAttribute(fbank512_nemo_stats_kernel)"
         : is_auto(k) ? "hipFuncSetAttribute(w512_auto_kernel)" : is_stream(k) ? "hipFuncSetAttribute(fbank512_stream_kernel)" : k >= K512::kKaldiIo80 ? "hipFuncSetAttribute(fbank512_kaldi_io_kernel)"
         : is_io(k) ? "hipFuncSetAttribute(fbank512_nemo_io_kernel)" : info_of(k).f32 ? "hipFuncSetAttribute(fbank512_wave_kernel<float>, 12 waves)"
                    : "hipFuncSetAttribute(fbank512_wave_kernel, 8 / 4 waves)";
}
template <class P> const char *attr_name(K512 k, const P &) { return attr_name(k); }
const char *attr_name(K512, const FbankStatsRaggedParams &) { return "hipFuncSetAttribute(fbank512_nemo_stats_ragged_kernel)"; }
const char *attr_name(K512, const FbankNemoStreamParams &) { return "hipFuncSetAttribute(fbank512_nemo_stream_kernel)"; }
// one launch of a route with the parameters of its kernel's group; z: the object's LDS sizes
template <class P>
int launch512(const Launch512 &l, const P &p, const Lds512Sizes &z, int cus, hipStream_t s) {
    static std::atomic<uint64_t> attr_done[idx(K512::kEnd)];          // one bit per device: function attributes are per device (one array per parameter struct)
    const auto kernel = kernel512(l.kernel, p);
    if (!kernel) return fail(MELSPEC_ERR_INTERNAL, "launch512: the object has no kernel for this batch");
    if (int rc = allow_big_lds_once(attr_done[idx(l.kernel)], attr_name(l.kernel, p), kernel)) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid512(l, batch_of(p).n_units, cus)), dim3(l.waves * 64), lds512(l.lds, z), s, p);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// the tables' part of the fused kernels' parameters ...
void set_tables(FbankFastParams &fp, const FbankFastTables &ft, const DevBuf &blob) {
    fp.d_blob = static_cast<const uint32_t *>(blob.p);
    fp.blob_words = static_cast<int>(ft.blob.size());
    fp.mel_off_words = ft.mel_off_words;
    fp.slots = ft.slots;
}
// ... and what every object fills alike; the caller adds its own fields
FbankFastParams fast_params(const FbankFastTables &ft, const DevBuf &blob, const BatchDesc &desc, int shift, int n_mels) {
    FbankFastParams fp{};
    fp.b = desc;
    set_tables(fp, ft, blob);
    fp.shift = shift;
    fp.n_mels = n_mels;
    return fp;
}
// what a route asks of its kernel's parameters: an f32 kernel reads the f32 tables; RoundSync as the route has it
void apply_route(const Route512 &r, FbankFastParams &fp, const Fused512F32 &f32) {
    if (info_of(r.run.kernel).f32) set_tables(fp, f32.ft, f32.d_blob);
    if (r.sync_rounds != kSyncKeep) fp.b.sync_rounds = r.sync_rounds;
}
// an object's shape from its tables (shape512) with the decision its create call made (lab builds: MELSPEC_RUNTIME_LENS=1 forces the run-time loop)
template <class A, class B>
Fused512Shape shape_of(Flavor512 flavor, bool fused, int waves, const MelSlots &ms, Bank512 a, Bank512 b) {
    Fused512Shape s = shape512<A, B>(flavor, Reach512{fused, waves, 0}, ms, a, b, kFbSlots);
    if (lab_runtime_lens()) s.bank = Bank512::kRuntime;
    return s;
}

Fused512Shape w512_shape(const melspec_ctx *c) {
    Fused512Shape s = shape_of<LensSlaney80W, LensSlaney128>(Flavor512::kWhisper, c->fast512, c->waves512, c->ft512.slots, Bank512::kSlaney80W, Bank512::kSlaney128);
    s.f32_built = c->f512.ok; s.precision = c->precision; s.adaptive = c->fix.adaptive; s.auto_possible = c->fix.count.p != nullptr;
    return s;
}

// MELSPEC_PRECISION_AUTO at n_fft = 512: the voting f32 launch and, gated on its verdict, the f64 launch (w512_auto_kernel)
int launch_w512_auto(melspec_ctx *c, const Route512 &r, const FbankFastParams &fp64, const Lds512Sizes &z, hipStream_t stream) {
    const BatchDesc &desc = fp64.b;
    FixSink sink{};
    int rc = auto_sink(c, desc, stream, true, sink);
    if (rc) return rc;
    sink.tab = nullptr;
    const unsigned grid32 = grid512(r.vote, desc.n_units, c->dev.cus);
    W512AutoParams q{};
    q.f = fp64;
    set_tables(q.f, c->f512.ft, c->f512.d_blob);
    q.fix = sink_armed(c, sink, desc, grid32);
    q.fix.vote_groups = std::min<unsigned>(grid32, static_cast<unsigned>(c->dev.cus));
    if ((rc = launch512(r.vote, q, z, c->dev.cus, stream))) return rc;
    // the gated launch: this batch's verdict (its number is c->fix.seq) decides between every unit, the noted units and nothing
    W512AutoParams g{};
    g.f = fp64;
    FixSink stat{};
    stat.count = sink.count; stat.acc = sink.acc; stat.host = sink.host; stat.list = sink.list;
    g.fix = sink_armed(c, stat, desc, grid512(r.gated, desc.n_units, c->dev.cus));          // (a launch number of its own: the host tells the two reports apart by kStatFromGated)
    g.fix.frames |= kStatFromGated;
    g.gate = sink.decision;
    g.gate_seq = q.fix.seq;
    return launch512(r.gated, g, z, c->dev.cus, stream);
}
}  // namespace

namespace melspec {
namespace host {
bool w512_auto_ok(const melspec_ctx *c) { return w512_auto_ok(w512_shape(c)); }
const char *whisper512_kernel_name(const melspec_ctx *c) { return whisper512_kernel_name(w512_shape(c)); }

// the Whisper flavour of the 512-point kernel: launch_ctx's branch for the n_fft = 512 contexts
int launch_whisper512(melspec_ctx *c, const BatchDesc &desc, hipStream_t stream) {
    const Route512 r = route512(w512_shape(c), is_layout(desc) ? Batch512::kLayout : Batch512::kPlain);
    FbankFastParams fp = fast_params(c->ft512, c->d_blob512, desc, c->hop_size, c->n_mels);
    fp.use_log = 1; fp.use_power = 1;
    const Lds512Sizes z{c->lds512, c->f512.lds, c->n_mels};
    if (r.vote.kernel != K512::kNone && desc.n_units >= w512_auto_min_units(c->dev.cus)) return launch_w512_auto(c, r, fp, z, stream);
    apply_route(r, fp, c->f512);
    return launch512(r.run, fp, z, c->dev.cus, stream);
}
}  // namespace host
}  // namespace melspec

// ------------------------------------------------------------------------------------
// Kaldi fbank context
// ------------------------------------------------------------------------------------
struct melspec_fbank {
    DeviceInfo dev;
    melspec_fbank_config cfg{};
    int frame_len = 0, frame_shift = 0, fft_size = 0;
    hipStream_t stream = nullptr;
    bool fast = false;          // fused 512-point kernel (default Kaldi geometry) vs generic f64 kernel
    bool use_generic = false;   // melspec_fbank_use_generic: the direct-DFT kernel as the on-device cross-check
    RaggedScratch ragged;
    DevicePlan dplan;
    HostPipe pipe;              // melspec_fbank_compute_batch_host
    FbankFastTables ft;
    DevBuf d_blob;
    size_t fast_lds = 0;
    int waves = 4;
    GenericTables gt;
    DevBuf h2d, d2h;
    StreamBuf rows32;           // apply_cmn with f16 / bf16 rows out: the f32 rows between the fbank kernel and the CMN, then the caller's
                                //   output offsets of a ragged batch (frames * num_mel_bins * 4 + n_clips * 8 bytes)
};


namespace {
uint64_t fbank_frames(const melspec_fbank *fb, uint64_t n) {
    return n < static_cast<uint64_t>(fb->frame_len) ? 0 : 1 + (n - fb->frame_len) / fb->frame_shift;   // src/fbank.rs:147-151
}
}  // namespace

extern "C" {

void melspec_fbank_default_config(melspec_fbank_config *c) {
    if (!c) return;
    c->sample_rate = 16000.0; c->num_mel_bins = 80; c->frame_length_ms = 25.0; c->frame_shift_ms = 10.0;
    c->energy_floor = 0.0; c->use_log_fbank = 1; c->use_power = 1; c->preemphasis = 0.97; c->apply_cmn = 1;
    c->low_freq = 20.0; c->high_freq = 0.0;
}

int melspec_fbank_create(melspec_fbank **out, int device, const melspec_fbank_config *cfg) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(MELSPEC_ERR_INVALID_ARG, "cfg is NULL");
    if (!(cfg->sample_rate > 0.0) || cfg->num_mel_bins <= 0 || !(cfg->frame_length_ms > 0.0) || !(cfg->frame_shift_ms > 0.0))
        return fail(MELSPEC_ERR_INVALID_ARG, "sample_rate, num_mel_bins, frame length and shift must be positive");
    // FbankConfig::{frame_length_samples, frame_shift_samples, fft_size}  (src/fbank.rs:66-82)
    const int frame_len = static_cast<int>(std::llround((cfg->frame_length_ms / 1000.0) * cfg->sample_rate));
    const int frame_shift = static_cast<int>(std::llround((cfg->frame_shift_ms / 1000.0) * cfg->sample_rate));
    if (frame_len < 2 || frame_shift < 1) return fail(MELSPEC_ERR_INVALID_ARG, "frame length/shift round to zero samples");
    int fft_size = 1;
    while (fft_size < frame_len) fft_size <<= 1;
    if (fft_size > kMaxGenericFft || cfg->num_mel_bins > kMaxGenericMels)
        return fail(MELSPEC_ERR_UNSUPPORTED, "fft_size must be <= 4096 and num_mel_bins <= 1024");
    DeviceInfo info;
    int rc = pick_device(device, info);
    if (rc) return rc;
    melspec_fbank *fb = new (std::nothrow) melspec_fbank();
    if (!fb) return fail(MELSPEC_ERR_INTERNAL, "out of host memory");
    fb->dev = info; fb->cfg = *cfg; fb->frame_len = frame_len; fb->frame_shift = frame_shift; fb->fft_size = fft_size;
    auto bail = [&](int code) { melspec_fbank_destroy(fb); return code; };
    if (hipSetDevice(info.device) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipSetDevice failed"));
    if (hipStreamCreate(&fb->stream) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipStreamCreate failed"));
    const double high = cfg->high_freq == 0.0 ? cfg->sample_rate / 2.0 : cfg->high_freq;
    const int bins = fft_size / 2 + 1;
    // the fused kernel computes in f64 up to |X|^2 (an f32 build cannot hold 1e-4 on quiet mel bands, see fbank_wave.hpp)
    fb->fast = frame_len == 400 && fft_size == 512 &&
               build_fbank_fast_tables<double>(cfg->sample_rate, cfg->num_mel_bins, cfg->low_freq, high, cfg->use_power != 0, fb->ft);
    if (fb->fast) {
        const Reach512 reach = fused512_reach(Flavor512::kKaldi, fb->ft.blob.size() * 4);
        fb->waves = reach.waves;
        fb->fast_lds = reach.lds_bytes;
        fb->fast = reach.fused;
    }
    if (fb->fast && (rc = upload(fb->d_blob, fb->ft.blob))) return bail(rc);
    const std::vector<double> dense = kaldi_mel_filterbank(cfg->sample_rate, fft_size, cfg->num_mel_bins, cfg->low_freq, high);
    if ((rc = fb->gt.build(fft_size, frame_len, bins, povey_window(frame_len), dense, cfg->num_mel_bins, bins))) return bail(rc);
    if (fb->gt.lds_bytes > kLdsLimit) return bail(fail(MELSPEC_ERR_UNSUPPORTED, "geometry needs more LDS than one workgroup has"));
    if ((rc = generic_allow_lds())) return bail(rc);
    *out = fb;
    return MELSPEC_OK;
}

void melspec_fbank_destroy(melspec_fbank *fb) {
    if (!fb) return;
    if (fb->dev.device >= 0) (void)hipSetDevice(fb->dev.device);
    if (fb->stream) { (void)hipStreamSynchronize(fb->stream); (void)hipStreamDestroy(fb->stream); }
    fb->gt.release(); fb->d_blob.release(); fb->h2d.release(); fb->d2h.release(); fb->ragged.release(); fb->dplan.release(); fb->pipe.release();
    fb->rows32.release();
    delete fb;
}

size_t melspec_fbank_num_frames(const melspec_fbank *fb, size_t n_samples) {
    return fb ? static_cast<size_t>(fbank_frames(fb, n_samples)) : 0;
}
int melspec_fbank_num_mel_bins(const melspec_fbank *fb) { return fb ? fb->cfg.num_mel_bins : 0; }
int melspec_fbank_uses_fast_path(const melspec_fbank *fb) { return fb && fb->fast && !fb->use_generic ? 1 : 0; }
int melspec_fbank_use_generic(melspec_fbank *fb, int on) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    fb->use_generic = on != 0;
    fb->gt.force_generic = on == 2;      // 2: the workgroup-per-frame kernel also where pow2_frame_kernel would take the geometry
    return MELSPEC_OK;
}

static double fbank_floor(const melspec_fbank *fb) { return fb->cfg.energy_floor > 0.0 ? fb->cfg.energy_floor : static_cast<double>(FLT_EPSILON); }

static Fused512Shape fbank_shape(const melspec_fbank *fb) {
    Fused512Shape s = shape_of<LensKaldi80, LensKaldi40>(Flavor512::kKaldi, fb->fast && !fb->use_generic, fb->waves, fb->ft.slots, Bank512::kKaldi80, Bank512::kKaldi40);
    s.cmn_power = fb->cfg.apply_cmn && fb->cfg.use_power;
    return s;
}

// the fused kernels' parameters of a batch of this object
static FbankFastParams fbank_fast_params(const melspec_fbank *fb, const BatchDesc &desc) {
    FbankFastParams fp = fast_params(fb->ft, fb->d_blob, desc, fb->frame_shift, fb->cfg.num_mel_bins);
    fp.preemph = fb->cfg.preemphasis > 0.0 ? fb->cfg.preemphasis : 0.0;   // src/fbank.rs:172
    fp.floor_v = static_cast<float>(fbank_floor(fb));
    fp.use_log = fb->cfg.use_log_fbank;
    fp.use_power = fb->cfg.use_power;
    return fp;
}

// cmn_kernel's and cmn_io_kernel's shape: rows staged per chunk (0: the column form) and the dynamic LDS of a workgroup
static void cmn_shape(int nm, uint64_t fpc /* frames of the longest clip */, int &rows_per_chunk, size_t &lds) {
    // rows staged per chunk (a multiple of 4: the fold works on units of 4 frames): what fits one workgroup's LDS next to the means and
    // the run sums; two workgroups per CU when a whole clip fits half of it
    const size_t head = static_cast<size_t>((nm + 3) & ~3) * 9 * sizeof(float);
    const bool staged = nm <= 512;
    size_t budget = kLdsLimit - head - 256;
    if (fpc * static_cast<uint64_t>(nm) * sizeof(float) + head <= kLdsLimit / 2 - 256) budget = kLdsLimit / 2 - head - 256;
    uint64_t rows = (budget / (static_cast<size_t>(nm) * sizeof(float))) & ~3ull;
    if (rows > ((fpc + 3) & ~3ull)) rows = (fpc + 3) & ~3ull;
    rows_per_chunk = staged ? static_cast<int>(rows) : 0;
    lds = staged ? head + static_cast<size_t>(rows_per_chunk) * nm * sizeof(float)
                 : (static_cast<size_t>((nm + 3) & ~3) + 8 * 512 + 512) * sizeof(float);
}

// The CMN pass of a batch (walks clips, not units) on the f32 rows of desc.out: in place (d_means: the split output, see fbank_launch) or --
// out_dtype f16 / bf16, the rows being a scratch -- from there to the caller's rows at dst (ragged batches: clip c at d_dst_off[c]).
static int launch_cmn(melspec_fbank *fb, const BatchDesc &desc, uint32_t n_clips, uint64_t fpc, hipStream_t s, float *d_means,
                      void *dst = nullptr, int out_dtype = MELSPEC_OUT_F32, const uint64_t *d_dst_off = nullptr) {
    const int nm = fb->cfg.num_mel_bins;
    int rows_per_chunk;
    size_t lds;
    cmn_shape(nm, fpc, rows_per_chunk, lds);
    const unsigned grid = grid_for(n_clips, fb->dev.cus, 8);
    static std::atomic<uint64_t> attr_done[2];
    if (out_dtype == MELSPEC_OUT_F32) {
        CmnParams cp{};
        cp.b = desc; cp.n_mels = nm; cp.rows_per_chunk = rows_per_chunk; cp.d_means = d_means;
        if (int rc = allow_big_lds_once(attr_done[0], "hipFuncSetAttribute(cmn_kernel)", &cmn_kernel<512>)) return rc;
        hipLaunchKernelGGL(cmn_kernel<512>, dim3(grid), dim3(512), lds, s, cp);
    } else {
        CmnIoParams cp{};
        cp.b = desc; cp.dst = dst; cp.d_dst_off = d_dst_off; cp.n_mels = nm; cp.rows_per_chunk = rows_per_chunk;
        if (int rc = allow_big_lds_once(attr_done[1], "hipFuncSetAttribute(cmn_io_kernel)", &cmn_io_kernel<io_f16>, &cmn_io_kernel<io_bf16>)) return rc;
        hipLaunchKernelGGL(out_dtype == MELSPEC_OUT_F16 ? cmn_io_kernel<io_f16> : cmn_io_kernel<io_bf16>, dim3(grid), dim3(kCmnThreads), lds, s, cp);
    }
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// the scratch of a CMN call with 16-bit rows out on stream s: `floats` f32 rows and, behind them, `tail` 64-bit words
static int fbank_rows32(melspec_fbank *fb, uint64_t floats, size_t tail, hipStream_t s, float *&rows, uint64_t *&words) {
    const size_t row_bytes = (static_cast<size_t>(floats) * sizeof(float) + 15) & ~static_cast<size_t>(15);
    const int rc = fb->rows32.ensure(row_bytes + tail * sizeof(uint64_t) + 16, s);
    rows = static_cast<float *>(fb->rows32.p());
    words = reinterpret_cast<uint64_t *>(static_cast<char *>(fb->rows32.p()) + row_bytes);
    return rc;
}

// Kernels of one batch (uniform or ragged plan): the fused 512-point kernel or the generic one, then the CMN per clip -- or the
// workgroup-per-clip kernel with the normalisation inside.  fpc: frames of the longest clip (LDS budget of the CMN).
// io = 0: the f32 call; d_means not nullptr: its split output -- un-normalised rows + the clips' column means.
// io != 0 (an object that kaldi_io_ok): the plan is the f32 call's, sample offsets and strides in elements; always the two-kernel path.
// pl.desc.out is where the rows of the wave kernel go: the caller's buffer, or -- CMN with 16-bit rows out -- the scratch, from where
// cmn_io_kernel writes them to vd_out (ragged: at d_dst_off).
static int fbank_launch(melspec_fbank *fb, const BatchPlan &pl, uint32_t n_clips, uint64_t fpc, hipStream_t s, int io = 0, float *d_means = nullptr,
                        void *vd_out = nullptr, const uint64_t *d_dst_off = nullptr) {
    const int nm = fb->cfg.num_mel_bins, out_dtype = io >> 4;
    const bool split = out_dtype != MELSPEC_OUT_F32 && fb->cfg.apply_cmn;
    int rc = MELSPEC_OK;
    if (fb->fast && !fb->use_generic) {
        const Fused512Shape shape = fbank_shape(fb);
        const FbankFastParams fp = fbank_fast_params(fb, pl.desc);
        const Lds512Sizes z{fb->fast_lds, 0, nm};
        // many clips of one length + CMN: the workgroup-per-clip kernel with the normalisation inside (fbank512_clip_kernel) when the
        // clips fill the CUs evenly enough (lab builds: MELSPEC_FB_CLIP=0 keeps the two kernels)
        static const bool clip_on = lab_int("MELSPEC_FB_CLIP", 1, 0, 1) != 0;
        const uint32_t cus = static_cast<uint32_t>(fb->dev.cus);
        const bool ragged_by_clip = pl.desc.d_order != nullptr;       // fbank_ragged decided (and checked the alignment)
        if (!io && clip_on && (ragged_by_clip ||
            (clip_shape_ok(shape, nm) && pl.desc.d_unit_prefix == nullptr && (reinterpret_cast<uintptr_t>(pl.desc.out) & 15) == 0 && pl.desc.out_stride % 4 == 0 &&
             clip_uniform_ok(n_clips, cus)))) {
            const Route512 r = route512(shape, ragged_by_clip ? Batch512::kClipRagged : Batch512::kClipUniform);
            if (lds512(r.run.lds, z) <= kLdsLimit) {
                FbankClipParams q{};
                q.f = fp;
                q.frames = fpc;
                static const int clip_skip = lab_int("MELSPEC_FB_CLIP_SKIP", 0, 0, 15);
                q.lab_skip = clip_skip;
                q.d_means = d_means;
                return launch512(r.run, q, z, fb->dev.cus, s);
            }
        }
        // (F32 samples, f32 rows into the scratch) is the f32 call's kernel
        const int kio = split ? io & 15 : io;
        const Route512 r = route512(shape, kio ? Batch512::kIo : is_layout(pl.desc) ? Batch512::kLayout : Batch512::kPlain, kio);
        rc = launch512(r.run, fp, z, fb->dev.cus, s);
        // the CMN pass below walks clips, not units
    } else {
        rc = launch_generic(fb->gt, pl.desc, fb->frame_shift, 1, fb->cfg.use_log_fbank, fb->cfg.use_power,
                            fb->cfg.preemphasis, fbank_floor(fb), fb->dev.cus, s);
    }
    if (rc || !fb->cfg.apply_cmn) return rc;
    if (split) return launch_cmn(fb, pl.desc, n_clips, fpc, s, nullptr, vd_out, out_dtype, d_dst_off);
    return launch_cmn(fb, pl.desc, n_clips, fpc, s, d_means);          // in place ((S16, F32): the f32 rows are the caller's)
}

// The uniform batch of melspec_fbank_compute_uniform_device, of its split form (d_means) and of its _io form.  io = pcm_dtype |
// out_dtype << 4 (fbank_io_args): 0 is the f32 call and launches exactly what it always did; otherwise vd_pcm / vd_out are int16 samples
// / f16, bf16 rows and the plan counts elements.
static int fbank_uniform(melspec_fbank *fb, const void *vd_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips, void *vd_out, void *stream, int io,
                         float *d_means = nullptr) {
    if (n_clips == 0) return MELSPEC_OK;
    const uint64_t fpc = fbank_frames(fb, clip_len);
    const int nm = fb->cfg.num_mel_bins;
    if (fpc == 0) {                     // zeros((0, num_mel_bins)), src/fbank.rs:147-149: no rows; the mean of nothing is reported as 0
        if (!d_means) return MELSPEC_OK;
        HIP_TRY(hipSetDevice(fb->dev.device));
        HIP_TRY(hipMemsetAsync(d_means, 0, static_cast<size_t>(n_clips) * nm * sizeof(float), stream ? static_cast<hipStream_t>(stream) : fb->stream));
        return MELSPEC_OK;
    }
    if (!vd_pcm || !vd_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    if (io && io_misaligned(vd_pcm, vd_out, io)) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type");
    HIP_TRY(hipSetDevice(fb->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fb->stream;
    const bool fused = fb->fast && !fb->use_generic;
    float *d_rows = static_cast<float *>(vd_out);
    // 16-bit rows cannot have their means subtracted in place: the wave kernel then writes f32 rows into the object's scratch
    if ((io >> 4) != MELSPEC_OUT_F32 && fb->cfg.apply_cmn) {
        uint64_t *words;
        if (int rc = fbank_rows32(fb, static_cast<uint64_t>(n_clips) * fpc * nm, 0, s, d_rows, words)) return rc;
    }
    const BatchPlan pl = plan_uniform(static_cast<const float *>(vd_pcm), d_rows, clip_stride, fpc, n_clips, nm, fused ? kFbFPW : 1);
    return fbank_launch(fb, pl, n_clips, fpc, s, io, d_means, vd_out, nullptr);
}

int melspec_fbank_compute_uniform_device(melspec_fbank *fb, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                         uint32_t n_clips, float *d_out, void *stream) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    return fbank_uniform(fb, d_pcm, clip_stride, clip_len, n_clips, d_out, stream, 0);
}

int melspec_fbank_compute_uniform_device_split(melspec_fbank *fb, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                               uint32_t n_clips, float *d_rows, float *d_means, void *stream) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    if (!fb->cfg.apply_cmn) return fail(MELSPEC_ERR_INVALID_ARG, "the split output is the CMN's two halves: FbankConfig::apply_cmn is off");
    if (n_clips == 0) return MELSPEC_OK;
    if (!d_means) return fail(MELSPEC_ERR_INVALID_ARG, "d_means is NULL");
    return fbank_uniform(fb, d_pcm, clip_stride, clip_len, n_clips, d_rows, stream, 0, d_means);
}

// Fbank::compute per clip of any length (src/fbank.rs:141): clip c = vd_pcm[h_offsets[c] .. + h_lengths[c]) -> its frames at
// vd_out + h_out_offsets[c] elements (NULL: packed); CMN per clip.  io: as in fbank_uniform; an _io batch runs on the two-kernel path
// (the wave-owned kernel, then the CMN per clip), whatever its shape.  d_means (io = 0): the split output, as in fbank_launch -- the rows
// stay un-normalised and the clips' column means go to d_means[clip][num_mel_bins]; a clip without a frame gets +0.0 there (neither the
// plan's order nor cmn_kernel visits it).
static int fbank_ragged(melspec_fbank *fb, const void *vd_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips, void *vd_out,
                        const uint64_t *h_out_offsets, void *stream, int io, float *d_means = nullptr) {
    if (n_clips == 0) return MELSPEC_OK;
    if (!h_offsets || !h_lengths) return fail(MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL");
    std::vector<uint64_t> frames(n_clips);
    uint64_t total = 0, longest = 0;
    for (uint32_t i = 0; i < n_clips; ++i) { frames[i] = fbank_frames(fb, h_lengths[i]); total += frames[i]; longest = std::max(longest, frames[i]); }
    if (total == 0) return MELSPEC_OK;
    if (!vd_pcm || !vd_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    if (io && io_misaligned(vd_pcm, vd_out, io)) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type");
    HIP_TRY(hipSetDevice(fb->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fb->stream;
    const bool fused = fb->fast && !fb->use_generic;
    const int nm = fb->cfg.num_mel_bins;
    int rc;
    float *d_rows = static_cast<float *>(vd_out);
    // CMN with 16-bit rows: the wave kernel writes f32 rows, packed in clip order, into the scratch (fbank_uniform); the caller's own
    // output offsets travel behind them
    const bool split = (io >> 4) != MELSPEC_OUT_F32 && fb->cfg.apply_cmn;
    const uint64_t *d_own = nullptr;
    if (split) {
        uint64_t *words;
        if ((rc = fbank_rows32(fb, total * static_cast<uint64_t>(nm), h_out_offsets ? n_clips : 0, s, d_rows, words))) return rc;
        if (h_out_offsets) {
            HIP_TRY(hipMemcpyAsync(words, h_out_offsets, static_cast<size_t>(n_clips) * sizeof(uint64_t), hipMemcpyHostToDevice, s));    // pageable source: staged before the call returns
            d_own = words;
        }
    }
    // whole clips per workgroup (fbank512_clip_kernel) when the batch can keep every CU busy (clip_ragged_ok); outputs at 16-byte offsets
    // (packed outputs of n_mels % 4 == 0 are)
    bool by_clip = !io && clip_shape_ok(fbank_shape(fb), nm) && (reinterpret_cast<uintptr_t>(vd_out) & 15) == 0 &&
                   clip_ragged_ok(n_clips, static_cast<uint32_t>(fb->dev.cus), longest, total);
    if (by_clip && h_out_offsets)
        for (uint32_t i = 0; i < n_clips && by_clip; ++i) by_clip = h_out_offsets[i] % 4 == 0;
    BatchPlan pl;
    RaggedSlot *slot = nullptr;
    if (d_means && std::find(frames.begin(), frames.end(), uint64_t{0}) != frames.end())
        HIP_TRY(hipMemsetAsync(d_means, 0, static_cast<size_t>(n_clips) * nm * sizeof(float), s));
    rc = plan_ragged(fb->ragged, s, static_cast<const float *>(vd_pcm), d_rows, h_offsets, frames, split ? nullptr : h_out_offsets, n_clips, nm, fused ? kFbFPW : 1, pl, slot, by_clip);
    if (!rc) rc = fbank_launch(fb, pl, n_clips, longest, s, io, d_means, vd_out, d_own ? d_own : pl.desc.d_out_off);
    plan_ragged_done(slot, s);
    return rc;
}

int melspec_fbank_compute_ragged_device(melspec_fbank *fb, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                        uint32_t n_clips, float *d_out, const uint64_t *h_out_offsets, void *stream) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    return fbank_ragged(fb, d_pcm, h_offsets, h_lengths, n_clips, d_out, h_out_offsets, stream, 0);
}

// the verdict of an argument check of the split calls as the call's status (the unsupported object is worded by the _split_io calls)
static int fbank_split_verdict(const FbankSplitArgs &a) {
    if (a.verdict != kFbankSplitFail) return MELSPEC_OK;
    return a.msg ? fail(a.status, a.msg) : a.status;
}
// no clip of the batch has a frame: there are no rows, and the mean of nothing is reported as +0.0 (melspec_fbank_compute_uniform_device_split)
static int fbank_split_zero_means(melspec_fbank *fb, float *d_means, uint32_t n_clips, void *stream) {
    HIP_TRY(hipSetDevice(fb->dev.device));
    HIP_TRY(hipMemsetAsync(d_means, 0, static_cast<size_t>(n_clips) * fb->cfg.num_mel_bins * sizeof(float), stream ? static_cast<hipStream_t>(stream) : fb->stream));
    return MELSPEC_OK;
}
static uint64_t fbank_total_frames(const melspec_fbank *fb, const uint64_t *h_lengths, uint32_t n_clips) {
    uint64_t total = 0;
    for (uint32_t i = 0; i < n_clips; ++i) total += fbank_frames(fb, h_lengths[i]);
    return total;
}

// The split output of a ragged batch: melspec_fbank_compute_ragged_device's routing with d_means threaded through -- large batches by clip
// (fbank512_clip_kernel publishes the means), everything else through the wave kernel (or the generic one) and cmn_kernel, which then
// writes the means and leaves the rows.  Both sum by the fixed tree: the bits do not depend on the route.
int melspec_fbank_compute_ragged_device_split(melspec_fbank *fb, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                              float *d_rows, const uint64_t *h_rows_offsets, float *d_means, void *stream) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    const uint64_t total = n_clips && h_offsets && h_lengths ? fbank_total_frames(fb, h_lengths, n_clips) : 0;
    const FbankSplitArgs a = fbank_split_args(fb->cfg.apply_cmn != 0, true, true, n_clips, h_offsets, h_lengths, total, d_pcm, d_rows, d_means, 0);
    if (a.verdict == kFbankSplitZero) return fbank_split_zero_means(fb, d_means, n_clips, stream);
    if (a.verdict != kFbankSplitGo) return fbank_split_verdict(a);
    return fbank_ragged(fb, d_pcm, h_offsets, h_lengths, n_clips, d_rows, h_rows_offsets, stream, 0, d_means);
}

// The same with the clip table in device memory (see melspec_compute_ragged_device_desc).
int melspec_fbank_compute_ragged_device_desc(melspec_fbank *fb, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                             uint32_t n_clips, float *d_out, const uint64_t *d_out_offsets, uint64_t max_total_frames,
                                             void *stream) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    if (n_clips == 0 || max_total_frames == 0) return MELSPEC_OK;
    if (!d_pcm || !d_out || !d_offsets || !d_lengths) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    HIP_TRY(hipSetDevice(fb->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fb->stream;
    const bool fused = fb->fast && !fb->use_generic;
    BatchPlan pl;
    int rc = plan_ragged_device(fb->dplan, s, d_pcm, d_out, d_offsets, d_lengths, d_out_offsets, n_clips, static_cast<uint64_t>(fb->frame_len),
                                static_cast<uint64_t>(fb->frame_shift), static_cast<uint32_t>(fb->cfg.num_mel_bins), fused ? kFbFPW : 1,
                                max_total_frames, pl);
    if (rc) return rc;
    return fbank_launch(fb, pl, n_clips, max_total_frames, s);
}

int melspec_fbank_release_scratch(melspec_fbank *fb) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    HIP_TRY(hipSetDevice(fb->dev.device));
    HIP_TRY(hipStreamSynchronize(fb->stream));
    if (int rc = fb->rows32.release_after(fb->stream)) return rc;
    fb->pipe.release(); fb->ragged.release(); fb->dplan.release(); fb->h2d.release(); fb->d2h.release();
    return MELSPEC_OK;
}

int melspec_fbank_synchronize(melspec_fbank *fb, void *stream) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    HIP_TRY(hipSetDevice(fb->dev.device));
    HIP_TRY(hipStreamSynchronize(stream ? static_cast<hipStream_t>(stream) : fb->stream));
    return MELSPEC_OK;
}

// Fbank::compute on many host clips in one call: whole clips (the CMN is per clip) through the host pipeline, one ragged launch per chunk.
int melspec_fbank_compute_batch_host(melspec_fbank *fb, const float *samples, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_clips,
                                     float *out, const uint64_t *out_offsets, size_t out_capacity_floats, uint64_t *total_frames) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    if (total_frames) *total_frames = 0;
    std::vector<HostSeg> segs;
    uint64_t total;
    if (int rc = host_segments(samples, offsets, lengths, n_clips, out, out_offsets, out_capacity_floats, static_cast<uint64_t>(fb->cfg.num_mel_bins),
                               [fb](uint64_t n) { return fbank_frames(fb, n); }, segs, total)) return rc;
    if (total_frames) *total_frames = total;
    if (total == 0) return MELSPEC_OK;
    HIP_TRY(hipSetDevice(fb->dev.device));
    return host_pipe_run(fb->pipe, segs, fb->cfg.num_mel_bins, fb->stream,
                         [fb](const float *d_in, const uint64_t *offs, const uint64_t *lens, uint32_t n, float *d_out, const uint64_t *ooffs, hipStream_t s) {
                             return melspec_fbank_compute_ragged_device(fb, d_in, offs, lens, n, d_out, ooffs, s);
                         });
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// NeMo / Parakeet frontend context (BatchLogMelSpectrogram, src/mel.rs:239-396)
// ------------------------------------------------------------------------------------
struct melspec_blm {
    DeviceInfo dev;
    melspec_blm_config cfg{};
    hipStream_t stream = nullptr;
    bool fast = false;          // fused 512-point kernel (n_fft 512 / win_length 400) vs the generic f64 kernel (any validated config)
    GenericTables gt;
    RaggedScratch ragged;
    StreamBuf aux;              // ragged batches: per-clip sample counts and valid frames, the normaliser's group counter
    DevicePlan dplan;           // melspec_blm_compute_ragged_device_desc: the plan and that block, written by blm_plan_ragged_device_kernel
    FbankFastTables ft;
    DevBuf d_blob;
    size_t fast_lds = 0;
    int waves = 4;
    int precision = MELSPEC_PRECISION_AUTO;     // melspec_blm_set_precision
    Fused512F32 f32;            // MELSPEC_PRECISION_F32: the reference's own arithmetic type for this frontend (src/mel.rs:251-252,356-357)
    DevBuf h2d, d2h;
    HostPipe pipe;              // melspec_blm_compute_batch_host
    StreamBuf rows32;           // normalize_per_feature with f16 / bf16 rows out: the f32 rows between the mel kernel and the normaliser
                                //   (n_clips * n_mels * cols * 4 bytes)
    StreamBuf stats;            // the split output: the per-block partials between the mel kernel and blm_stats_finish_kernel
                                //   (n_clips * ceil(cols / 32 or 48) * n_mels * 8 bytes)
};

namespace {
uint64_t blm_valid_frames(const melspec_blm *b, uint64_t n) {       // src/mel.rs:326-332,387-395
    if (n == 0) return 0;
    if (b->cfg.center) return n / b->cfg.hop_length + 1;
    if (n < static_cast<uint64_t>(b->cfg.n_fft)) return 0;
    return (n - b->cfg.n_fft) / b->cfg.hop_length + 1;
}
uint64_t blm_padded(const melspec_blm *b, uint64_t frames) {         // pad_len, src/mel.rs:751-756
    const uint64_t p = b->cfg.pad_to;
    return p == 0 ? frames : (frames + p - 1) / p * p;
}

Fused512Shape blm_shape(const melspec_blm *b) {
    Fused512Shape s = shape_of<LensSlaney128, LensSlaney80>(Flavor512::kNemo, b->fast, b->waves, b->ft.slots, Bank512::kSlaney128, Bank512::kSlaney80);
    s.f32_built = b->f32.ok; s.precision = b->precision;
    return s;
}

// ---- int16 PCM in / f16, bf16 rows out (melspec_blm_compute_*_io) ---------------------------------------------------------------------
// the contexts whose kernels have the instantiations: the fused geometry on eight f64 waves with one of the compile-time Slaney banks
bool blm_io_ok(const melspec_blm *b) { return nemo_io_ok(blm_shape(b)); }
// 0: go on (io = pcm_dtype | out_dtype << 4, 0 for (F32, F32)); otherwise the status to return
int blm_io_args(const melspec_blm *b, int pcm_dtype, int out_dtype, int &io) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (int rc = io_dtypes(pcm_dtype, out_dtype, io)) return rc;
    if (io && !blm_io_ok(b)) {
        g_last_error = "int16 PCM / f16, bf16 rows are computed by the n_fft = 512 / win_length = 400 frontend with the 80- or 128-mel Slaney bank only; this context is n_fft = " +
                       std::to_string(b->cfg.n_fft) + ", win_length = " + std::to_string(b->cfg.win_length) + ", n_mels = " + std::to_string(b->cfg.n_mels) +
                       (b->fast ? " (another filterbank)" : "");
        return MELSPEC_ERR_UNSUPPORTED;
    }
    return MELSPEC_OK;
}

// the f32 rows of a normalised call with 16-bit rows out: `floats` of them, on stream s
int blm_rows32(melspec_blm *b, uint64_t floats, hipStream_t s, float *&rows) {
    // + 16: the normaliser reads whole 16-byte granules, the last row's last one included
    const int rc = b->rows32.ensure(static_cast<size_t>(floats) * sizeof(float) + 16, s);
    rows = static_cast<float *>(b->rows32.p());
    return rc;
}

// rows staged per workgroup (`per`, 0: a row does not fit), the row stride in LDS and the workgroups per CU of the normalisers.  The
// number of rows per workgroup decides how many threads share a row's sum of squares, i.e. the order of that sum: the in-place f32
// passes and the passes that write 16-bit rows take their shape from the same function, whatever else the latter keep in LDS, so that the
// statistics of a 16-bit call are those of the f32 call bit for bit.
// uniform batches, rows of `valid` frames: four workgroups of <= 38 KB per CU measured best (1024 x 10 s x 128 mels, ms per call incl. the
// 0.72 ms mel kernel: 150 KB x 1: 1.72, 76 x 2: 1.45, 50 x 3: 1.34, 38 x 4: 1.28, 25 x 6: 1.68); MELSPEC_NORM_KB / MELSPEC_NORM_PER_CU override
void blm_norm_shape_uniform(uint64_t valid, size_t &stride, size_t &per, int &per_cu) {
    stride = (static_cast<size_t>(valid) + 3 + 31) & ~static_cast<size_t>(31);  // whole groups of 32 floats (a row starts up to 3 floats into its first granule) ...
    if ((stride / 4) % 2 == 0) stride += 4;                                       // ... and 4 * odd
    static const int norm_kb = lab_int("MELSPEC_NORM_KB", 38, 8, 158);
    static const int norm_per_cu = lab_int("MELSPEC_NORM_PER_CU", 4, 1, 16);
    const size_t budget = static_cast<size_t>(norm_kb) * 1024 - (64 * 2 + kBlmNormThreads) * sizeof(float);
    per = budget / (stride * sizeof(float));
    per_cu = norm_per_cu;
    if (per < 4) {                            // long rows (> ~25 s): one workgroup per CU with the whole LDS, up to ~6 min per row
        per = (static_cast<size_t>(150) * 1024) / (stride * sizeof(float));
        per_cu = 1;
    }
    if (per > 64) per = 64;
}
// ragged batches: blm_norm_shape_ragged (blm_desc_plan.hpp: the planner kernel of the _desc call evaluates it too) -- rows staged whole in
// LDS like the uniform pass (sized for the longest clip), groups of rows from a counter
static_assert(kBlmDescNormThreads == kBlmNormThreads && kBlmDescFramesPerUnit == kFbFPW && kBlmDescUnitBlock == kUnitBlock, "blm_desc_plan.hpp restates the kernels' constants");

// the fused kernels' parameters of a batch of this context (fbank_fast_params' counterpart); the caller adds what its kind of batch has
FbankFastParams blm_fast_params(const melspec_blm *b, const BatchDesc &desc) {
    FbankFastParams fp = fast_params(b->ft, b->d_blob, desc, b->cfg.hop_length, b->cfg.n_mels);
    fp.preemph = b->cfg.preemphasis;
    fp.floor_v = b->cfg.log_zero_guard;
    fp.use_log = 1; fp.use_power = 1;
    fp.org0 = b->cfg.center ? -200 : 56;      // tap 0 of the window sits at position (512-400)/2 of the frame
    return fp;
}
Lds512Sizes blm_lds(const melspec_blm *b) { return Lds512Sizes{b->fast_lds, b->f32.lds, b->cfg.n_mels}; }

// the mel kernel of a batch: the (sample, row) combination io, the f32 kernel, the f64 kernel of a compile-time bank or of any bank
int launch_nemo_mel(melspec_blm *b, FbankFastParams fp, int io, hipStream_t s) {
    const Route512 r = route512(blm_shape(b), io ? Batch512::kIo : Batch512::kLayout, io);
    apply_route(r, fp, b->f32);
    return launch512(r.run, fp, blm_lds(b), b->dev.cus, s);
}

// The rows a normaliser works on: f32 rows read at src and written at dst as out_dtype -- MELSPEC_OUT_F32: in place (dst == src), f16 / bf16:
// split, src being the context's scratch.  Ragged batches: clip c at d_src_off[c] / d_dst_off[c] (in place: the same), its row width and
// valid frames in d_cols / d_valid.
struct BlmNormRows {
    const float *src;
    void *dst;
    int out_dtype;
    uint32_t n_clips;
    const uint64_t *d_src_off, *d_dst_off, *d_cols, *d_valid;
};

// rows too long for LDS: one thread per row from HBM (blm_normalize_kernel / blm_normalize_io_kernel with rows_per_group == 0); uniform
// batches: rows of `valid` frames in `cols` columns.  The caller looks at hipGetLastError.
void launch_blm_norm_slow(melspec_blm *b, const BlmNormRows &r, uint64_t cols, uint64_t valid, hipStream_t s) {
    const int nm = b->cfg.n_mels;
    const uint64_t rows = static_cast<uint64_t>(r.n_clips) * nm;
    const dim3 grid(grid_for((rows + kBlmNormThreads - 1) / kBlmNormThreads, b->dev.cus, 4));
    if (r.out_dtype == MELSPEC_OUT_F32) {
        BlmNormParams np{};
        np.out = static_cast<float *>(r.dst); np.clip_stride = cols * static_cast<uint64_t>(nm); np.row_w = cols; np.valid = valid;
        np.n_clips = r.n_clips; np.n_mels = nm; np.rows_per_group = 0; np.fold_sel = -1;
        np.d_out_off = r.d_dst_off; np.d_cols = r.d_cols; np.d_valid = r.d_valid;
        hipLaunchKernelGGL(blm_normalize_kernel, grid, dim3(kBlmNormThreads), 0, s, np);
    } else {
        BlmNormIoParams np{};
        np.src = r.src; np.dst = r.dst; np.row_w = cols; np.valid = valid; np.n_clips = r.n_clips; np.n_mels = nm; np.rows_per_group = 0;
        np.d_src_off = r.d_src_off; np.d_dst_off = r.d_dst_off; np.d_cols = r.d_cols; np.d_valid = r.d_valid;
        hipLaunchKernelGGL(r.out_dtype == MELSPEC_OUT_F16 ? blm_normalize_io_kernel<io_f16> : blm_normalize_io_kernel<io_bf16>, grid, dim3(kBlmNormThreads), 0, s, np);
    }
}

// normalize_per_feature over a uniform batch: rows of `valid` frames in `cols` columns
int launch_blm_norm(melspec_blm *b, const BlmNormRows &r, uint64_t cols, uint64_t valid, hipStream_t s) {
    const int nm = b->cfg.n_mels;
    const uint64_t rows = static_cast<uint64_t>(r.n_clips) * nm;
    const bool split = r.out_dtype != MELSPEC_OUT_F32;
    size_t stride, per;
    int per_cu;
    blm_norm_shape_uniform(valid, stride, per, per_cu);
    static std::atomic<uint64_t> attr_done[2];
    if (int rc = split ? allow_big_lds_once(attr_done[1], "hipFuncSetAttribute(blm_normalize_io_kernel)", &blm_normalize_io_kernel<io_f16>, &blm_normalize_io_kernel<io_bf16>)
                       : allow_big_lds_once(attr_done[0], "hipFuncSetAttribute(blm_normalize_kernel)", &blm_normalize_kernel))
        return rc;
    if (per == 0) {
        launch_blm_norm_slow(b, r, cols, valid, s);
        HIP_TRY(hipGetLastError());
        return MELSPEC_OK;
    }
    const size_t lds = (per * stride + 2 * per + kBlmNormThreads) * sizeof(float);
    const unsigned g2 = grid_for((rows + per - 1) / per, b->dev.cus, per_cu);
    if (split) {
        BlmNormIoParams np{};
        np.src = r.src; np.dst = r.dst; np.row_w = cols; np.valid = valid; np.n_clips = r.n_clips; np.n_mels = nm;
        np.rows_per_group = static_cast<int>(per);
        np.lds_stride = static_cast<int>(stride);
        hipLaunchKernelGGL(r.out_dtype == MELSPEC_OUT_F16 ? blm_normalize_io_kernel<io_f16> : blm_normalize_io_kernel<io_bf16>, dim3(g2), dim3(kBlmNormThreads), lds, s, np);
        HIP_TRY(hipGetLastError());
        return MELSPEC_OK;
    }
    BlmNormParams np{};
    np.out = static_cast<float *>(r.dst); np.clip_stride = cols * static_cast<uint64_t>(nm); np.row_w = cols; np.valid = valid;
    np.n_clips = r.n_clips; np.n_mels = nm;
    static const int fold_sel = lab_int("MELSPEC_NORM_FOLD", -1, -1, 12);
    np.fold_sel = fold_sel;
    static const int norm_skip = lab_int("MELSPEC_NORM_SKIP", 0, 0, 7);
    np.lab_skip = norm_skip;
    np.rows_per_group = static_cast<int>(per);
    np.lds_stride = static_cast<int>(stride);
#ifdef MELSPEC_LAB
    static const int norm_dbg = lab_int("MELSPEC_NORM_DBG", 0, 0, 1);
    static uint64_t *d_dbg = nullptr;
    static int dbg_calls = 0;
    if (norm_dbg) {
        if (!d_dbg) HIP_TRY(hipMalloc(reinterpret_cast<void **>(&d_dbg), 64 * 8 * 8));
        HIP_TRY(hipMemsetAsync(d_dbg, 0, 64 * 8 * 8, s));
        np.dbg = d_dbg;
    }
#endif
    hipLaunchKernelGGL(blm_normalize_kernel, dim3(g2), dim3(kBlmNormThreads), lds, s, np);
#ifdef MELSPEC_LAB
    if (norm_dbg && ++dbg_calls == 20) {
        uint64_t h[64 * 8];
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(h, d_dbg, sizeof(h), hipMemcpyDeviceToHost));
        double sum[8] = {0};
        for (int b = 0; b < 64; ++b) for (int k = 0; k < 8; ++k) sum[k] += static_cast<double>(h[b * 8 + k]);
        std::fprintf(stderr, "norm phases, us per workgroup (mean of 64): load %.1f  mean %.1f  var %.1f  var-sum %.1f  store %.1f\n",
                     sum[1] / 64 / 100, sum[2] / 64 / 100, sum[3] / 64 / 100, sum[4] / 64 / 100, sum[5] / 64 / 100);
    }
#endif
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// ... over a ragged batch whose longest clip has `longest` valid frames; ctr: the group counter, zero at launch
int launch_blm_norm_ragged(melspec_blm *b, const BlmNormRows &r, uint64_t longest, unsigned *ctr, hipStream_t s) {
    const int nm = b->cfg.n_mels;
    const uint64_t rows = static_cast<uint64_t>(r.n_clips) * nm;
    const bool split = r.out_dtype != MELSPEC_OUT_F32;
    size_t stride, per;
    int per_cu;
    blm_norm_shape_ragged(longest, stride, per, per_cu);      // (the split pass's rows carry two more words each: <= 512 bytes)
    if (per < 1 || longest >= (1ull << 31)) {
        launch_blm_norm_slow(b, r, 0, 0, s);
        if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, split ? "blm_normalize_io_kernel launch failed" : "blm_normalize_kernel launch failed");
        return MELSPEC_OK;
    }
    static std::atomic<uint64_t> attr_done[2];
    if (int rc = split ? allow_big_lds_once(attr_done[1], "hipFuncSetAttribute(blm_normalize_ragged_io_kernel)", &blm_normalize_ragged_io_kernel<io_f16>,
                                            &blm_normalize_ragged_io_kernel<io_bf16>)
                       : allow_big_lds_once(attr_done[0], "hipFuncSetAttribute(blm_normalize_ragged_kernel)", &blm_normalize_ragged_kernel))
        return rc;
    const size_t lds = (per * stride + 2 * per + kBlmNormThreads + (split ? kBlmNormIoInfo : kBlmNormInfo) * per + 4) * sizeof(float);
    const unsigned g2 = grid_for((rows + per - 1) / per, b->dev.cus, per_cu);
    if (split) {
        BlmNormRaggedIoParams rp{};
        rp.src = r.src; rp.dst = r.dst; rp.d_src_off = r.d_src_off; rp.d_dst_off = r.d_dst_off; rp.d_cols = r.d_cols; rp.d_valid = r.d_valid;
        rp.n_clips = r.n_clips; rp.n_mels = nm; rp.rows_per_group = static_cast<int>(per); rp.lds_stride = static_cast<int>(stride);
        rp.ctr = ctr;
        hipLaunchKernelGGL(r.out_dtype == MELSPEC_OUT_F16 ? blm_normalize_ragged_io_kernel<io_f16> : blm_normalize_ragged_io_kernel<io_bf16>, dim3(g2), dim3(kBlmNormThreads), lds, s, rp);
    } else {
        BlmNormRaggedParams rp{};
        rp.out = static_cast<float *>(r.dst); rp.d_out_off = r.d_dst_off; rp.d_cols = r.d_cols; rp.d_valid = r.d_valid;
        rp.n_clips = r.n_clips; rp.n_mels = nm; rp.rows_per_group = static_cast<int>(per); rp.lds_stride = static_cast<int>(stride);
        rp.longest = static_cast<uint32_t>(longest);
        rp.ctr = ctr;
        hipLaunchKernelGGL(blm_normalize_ragged_kernel, dim3(g2), dim3(kBlmNormThreads), lds, s, rp);
    }
    if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, split ? "blm_normalize_ragged_io_kernel launch failed" : "blm_normalize_ragged_kernel launch failed");
    return MELSPEC_OK;
}

// ... in place over a batch planned on the device: `longest` is the valid frames of the caller's bound on a clip's samples, which sizes the
// launch; d_order: the order of a row's sum of squares, noted by the planner (blm_normalize_ragged_desc_kernel says what for)
int launch_blm_norm_ragged_desc(melspec_blm *b, float *rows_at, uint32_t n_clips, const BatchDesc &desc, const BlmDevicePlanAux &aux, uint64_t longest, hipStream_t s) {
    const int nm = b->cfg.n_mels;
    const uint64_t rows = static_cast<uint64_t>(n_clips) * nm;
    size_t stride, per;
    int per_cu;
    blm_desc_norm_launch(longest, stride, per, per_cu);
    BlmNormRaggedDescParams q{};
    BlmNormRaggedParams &rp = q.r;
    rp.out = rows_at; rp.d_out_off = desc.d_out_off; rp.d_cols = desc.d_frames; rp.d_valid = aux.d_valid;
    rp.n_clips = n_clips; rp.n_mels = nm;
    rp.ctr = aux.d_ctr;
    q.d_order = aux.d_order;
    if (per < 1 || longest >= (1ull << 31)) {
        hipLaunchKernelGGL(blm_normalize_ragged_desc_slow_kernel, dim3(grid_for((rows + kBlmNormThreads - 1) / kBlmNormThreads, b->dev.cus, 4)), dim3(kBlmNormThreads), 0, s, q);
        if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, "blm_normalize_ragged_desc_slow_kernel launch failed");
        return MELSPEC_OK;
    }
    static std::atomic<uint64_t> attr_done;
    if (int rc = allow_big_lds_once(attr_done, "hipFuncSetAttribute(blm_normalize_ragged_desc_kernel)", &blm_normalize_ragged_desc_kernel)) return rc;
    rp.rows_per_group = static_cast<int>(per); rp.lds_stride = static_cast<int>(stride);
    rp.longest = static_cast<uint32_t>(longest);
    const size_t lds = (per * stride + 2 * per + kBlmNormThreads + kBlmNormInfo * per + 4) * sizeof(float);
    hipLaunchKernelGGL(blm_normalize_ragged_desc_kernel, dim3(grid_for((rows + per - 1) / per, b->dev.cus, per_cu)), dim3(kBlmNormThreads), lds, s, q);
    if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, "blm_normalize_ragged_desc_kernel launch failed");
    return MELSPEC_OK;
}
}  // namespace

extern "C" {

void melspec_blm_default_config(melspec_blm_config *c) {
    if (!c) return;
    c->sample_rate = 16000; c->n_fft = 512; c->win_length = 400; c->hop_length = 160; c->n_mels = 80;
    c->f_min = 0.0; c->f_max = -1.0; c->htk = 0; c->norm = 1; c->preemphasis = 0.0f; c->center = 1;
    c->log_zero_guard = FLT_EPSILON; c->pad_to = 0; c->normalize_per_feature = 0;
}

int melspec_blm_create(melspec_blm **out, int device, const melspec_blm_config *cfg) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!cfg) return fail(MELSPEC_ERR_INVALID_ARG, "cfg is NULL");
    // validate_batch_config (src/mel.rs:656-683), same order and messages
    if (cfg->sample_rate <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: sample_rate must be > 0");
    if (cfg->n_fft <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: n_fft must be > 0");
    if (cfg->win_length <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: win_length must be > 0");
    if (cfg->win_length > cfg->n_fft) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: win_length must be <= n_fft");
    if (cfg->hop_length <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: hop_length must be > 0");
    if (cfg->n_mels <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: n_mels must be > 0");
    if (!std::isfinite(cfg->log_zero_guard) || cfg->log_zero_guard <= 0.0f)
        return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: log_zero_guard must be finite and > 0");
    if (cfg->pad_to < 0) return fail(MELSPEC_ERR_INVALID_ARG, "invalid log-mel config: pad_to must be >= 0");
    if (cfg->n_fft > kMaxGenericFft || cfg->n_mels > kMaxGenericMels)
        return fail(MELSPEC_ERR_UNSUPPORTED, "n_fft must be <= 4096 and n_mels <= 1024");
    DeviceInfo info;
    int rc = pick_device(device, info);
    if (rc) return rc;
    melspec_blm *b = new (std::nothrow) melspec_blm();
    if (!b) return fail(MELSPEC_ERR_INTERNAL, "out of host memory");
    b->dev = info; b->cfg = *cfg;
    auto bail = [&](int code) { melspec_blm_destroy(b); return code; };
    if (hipSetDevice(info.device) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipSetDevice failed"));
    if (hipStreamCreate(&b->stream) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipStreamCreate failed"));
    const double f_max = cfg->f_max > 0.0 ? cfg->f_max : cfg->sample_rate / 2.0;   // src/mel.rs:254
    // the NeMo / Parakeet geometry (n_fft 512, win_length 400) runs on the fused 512-point kernel; every other validated config
    // (src/mel.rs:248-280 accepts them all) on the generic f64 kernel
    b->fast = cfg->n_fft == 512 && cfg->win_length == 400 &&
              build_blm_fast_tables<double>(cfg->sample_rate, cfg->n_mels, cfg->f_min, f_max, cfg->htk != 0, cfg->norm != 0, b->ft);
    if (b->fast) {
        const Reach512 reach = fused512_reach(Flavor512::kNemo, b->ft.blob.size() * 4);      // (the RoundSync counters are part of the 8-or-4 question)
        b->waves = reach.waves;
        b->fast_lds = reach.lds_bytes;
        b->fast = reach.fused;
    }
    if (b->fast) {
        if ((rc = upload(b->d_blob, b->ft.blob))) return bail(rc);
        if (nemo_f32_bank(b->ft.slots) && build_blm_fast_tables<float>(cfg->sample_rate, cfg->n_mels, cfg->f_min, f_max, cfg->htk != 0, cfg->norm != 0, b->f32.ft) &&
            (rc = b->f32.finish(0, StagedRows<kFused512F32Waves>::bytes(cfg->n_mels)))) return bail(rc);
    } else {
        // the reference's f32 tables: symmetric Hann(win_length) centred in the n_fft frame (src/mel.rs:708-719), f32 weights
        const int N = cfg->n_fft, bins = N / 2 + 1;
        std::vector<double> win(static_cast<size_t>(N), 0.0);
        if (cfg->win_length > 1) {
            const int offset = (N - cfg->win_length) / 2;
            const float pi_f32 = 3.14159265358979323846f;
            for (int i = 0; i < cfg->win_length; ++i) {
                const float phase = (2.0f * pi_f32 * static_cast<float>(i)) / (static_cast<float>(cfg->win_length) - 1.0f);
                win[offset + i] = static_cast<double>(0.5f - (0.5f * std::cos(phase)));
            }
        }
        std::vector<double> dense = mel_filterbank(static_cast<double>(cfg->sample_rate), N, cfg->n_mels, cfg->f_min > 0.0 ? cfg->f_min : -1.0, f_max,
                                                   cfg->htk != 0, cfg->norm != 0);
        for (double &w : dense) w = static_cast<double>(static_cast<float>(w));
        if ((rc = b->gt.build(N, N, bins, win, dense, cfg->n_mels, bins))) return bail(rc);
        if (b->gt.lds_bytes > kLdsLimit) return bail(fail(MELSPEC_ERR_UNSUPPORTED, "geometry needs more LDS than one workgroup has"));
        if ((rc = generic_allow_lds())) return bail(rc);
    }
    *out = b;
    return MELSPEC_OK;
}

void melspec_blm_destroy(melspec_blm *b) {
    if (!b) return;
    if (b->dev.device >= 0) (void)hipSetDevice(b->dev.device);
    if (b->stream) { (void)hipStreamSynchronize(b->stream); (void)hipStreamDestroy(b->stream); }
    b->d_blob.release(); b->f32.d_blob.release(); b->h2d.release(); b->d2h.release(); b->gt.release(); b->ragged.release(); b->aux.release(); b->pipe.release(); b->rows32.release();
    b->stats.release(); b->dplan.release();
    delete b;
}

// F32: the reference's own arithmetic type for this frontend (f32 window, FFT, power and projection, src/mel.rs:251-252,356-357) on the
// f32 instantiation of the fused kernel -- as far from the f64 evaluation of the definition as upstream's own f32 code is (2.4e-4 on
// jfk_f32le.wav, 5e-4 on a chirp; tools/f32_512_probe.py).  AUTO / F64 (the default): f64 from the window to |X|^2, within 1e-4 of that
// evaluation on every input.  Contexts without an f32 kernel (other geometries, other banks) compute in f64 whatever the mode.
int melspec_blm_set_precision(melspec_blm *b, int mode) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (mode != MELSPEC_PRECISION_AUTO && mode != MELSPEC_PRECISION_F64 && mode != MELSPEC_PRECISION_F32)
        return fail(MELSPEC_ERR_INVALID_ARG, "precision must be MELSPEC_PRECISION_AUTO, _F64 or _F32");
    b->precision = mode;
    return MELSPEC_OK;
}
int melspec_blm_precision(const melspec_blm *b) {       // the arithmetic the next call will use: MELSPEC_PRECISION_F32 or _F64
    return b && b->precision == MELSPEC_PRECISION_F32 && b->fast && b->f32.ok ? MELSPEC_PRECISION_F32 : MELSPEC_PRECISION_F64;
}

size_t melspec_blm_num_frames(const melspec_blm *b, size_t n) { return b ? static_cast<size_t>(blm_valid_frames(b, n)) : 0; }
size_t melspec_blm_padded_frames(const melspec_blm *b, size_t n) { return b ? static_cast<size_t>(blm_padded(b, blm_valid_frames(b, n))) : 0; }

// The uniform batch of melspec_blm_compute_uniform_device and of its _io form.  io = pcm_dtype | out_dtype << 4 (blm_io_args): 0 is the
// f32 call and launches exactly what it always did; otherwise vd_pcm / vd_out are int16 samples / f16, bf16 rows and the plan counts elements.
static int blm_uniform(melspec_blm *b, const void *vd_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips, void *vd_out, void *stream, int io) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (n_clips == 0) return MELSPEC_OK;
    const uint64_t valid = blm_valid_frames(b, clip_len), cols = blm_padded(b, valid);
    if (cols == 0) return MELSPEC_OK;
    if (!vd_pcm || !vd_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    if (io && io_misaligned(vd_pcm, vd_out, io)) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    const int nm = b->cfg.n_mels;
    int rc;
    const float *d_pcm = static_cast<const float *>(vd_pcm);
    float *d_out = static_cast<float *>(vd_out);
    // 16-bit rows cannot be normalised in place: the mel kernel then writes f32 rows into the context's scratch and the normaliser reads them there
    const int out_dtype = io >> 4;
    const bool split = out_dtype != 0 && b->cfg.normalize_per_feature && valid > 0;
    if (split) {
        if ((rc = blm_rows32(b, static_cast<uint64_t>(n_clips) * nm * cols, s, d_out))) return rc;
        io &= 15;
    }
    if (!b->fast) {
        const BatchPlan pl = plan_uniform(d_pcm, d_out, clip_stride, valid, n_clips, nm, 1, cols, true);
        rc = launch_generic(b->gt, pl.desc, b->cfg.hop_length, 2, 1, 1, static_cast<double>(b->cfg.preemphasis), static_cast<double>(b->cfg.log_zero_guard),
                            b->dev.cus, s, static_cast<long long>(clip_len), b->cfg.center ? b->cfg.n_fft / 2 : 0);
        if (rc) return rc;
    } else {
        const BatchPlan pl = plan_uniform(d_pcm, d_out, clip_stride, valid, n_clips, nm, kFbFPW, cols, true);
        FbankFastParams fp = blm_fast_params(b, pl.desc);
        // feature-major store: waves holding adjacent units are kept in step (RoundSync); measured best for this kernel, see DESIGN 4.2b
        if (fp.b.sync_rounds < 0) fp.b.sync_rounds = kNemoSync;
        fp.clip_len = static_cast<long long>(clip_len);
        if ((rc = launch_nemo_mel(b, fp, io, s))) return rc;
    }
    if (b->cfg.normalize_per_feature && valid > 0)      // split: from the scratch to the caller's rows; otherwise in place
        return launch_blm_norm(b, BlmNormRows{d_out, split ? vd_out : d_out, split ? out_dtype : MELSPEC_OUT_F32, n_clips, nullptr, nullptr, nullptr, nullptr}, cols, valid, s);
    return MELSPEC_OK;
}

int melspec_blm_compute_uniform_device(melspec_blm *b, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                       uint32_t n_clips, float *d_out, void *stream) {
    return blm_uniform(b, d_pcm, clip_stride, clip_len, n_clips, d_out, stream, 0);
}

// BatchLogMelSpectrogram::compute per clip of any length (src/mel.rs:299-385) in one launch: clip c = d_pcm[h_offsets[c] .. + h_lengths[c])
// -> [n_mels][cols_c] floats at d_out + h_out_offsets[c] (NULL: packed in clip order), cols_c = melspec_blm_padded_frames(len_c).
// Fused kernel only (n_fft 512 / win_length 400).
// io: as in blm_uniform.
static int blm_ragged(melspec_blm *b, const void *vd_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips, void *vd_out,
                      const uint64_t *h_out_offsets, void *stream, int io) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (n_clips == 0) return MELSPEC_OK;
    if (!h_offsets || !h_lengths) return fail(MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL");
    if (!b->fast) return fail(MELSPEC_ERR_UNSUPPORTED, "ragged batches need the fused kernel (n_fft = 512, win_length = 400)");
    const float *d_pcm = static_cast<const float *>(vd_pcm);
    float *d_out = static_cast<float *>(vd_out);
    const int out_dtype = io >> 4;
    // 16-bit rows + normalisation: the mel kernel writes f32 rows, packed in clip order, into the context's scratch (blm_uniform); the
    // caller's own output offsets then travel behind the group counter
    const bool split = out_dtype != 0 && b->cfg.normalize_per_feature;
    const bool own_offsets = split && h_out_offsets != nullptr;
    // lengths, valid frames, the normaliser's group counter (0) [, the caller's output offsets]
    std::vector<uint64_t> cols(n_clips), aux(2 * static_cast<size_t>(n_clips) + 1 + (own_offsets ? n_clips : 0));
    uint64_t total = 0, longest = 0;
    for (uint32_t i = 0; i < n_clips; ++i) {
        const uint64_t valid = blm_valid_frames(b, h_lengths[i]);
        cols[i] = blm_padded(b, valid);
        aux[i] = h_lengths[i];
        aux[n_clips + i] = valid;
        total += cols[i];
        longest = std::max(longest, valid);
    }
    if (total == 0) return MELSPEC_OK;
    if (!d_pcm || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    if (io && io_misaligned(vd_pcm, vd_out, io)) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    const int nm = b->cfg.n_mels;
    int rc = b->aux.ensure(aux.size() * sizeof(uint64_t), s);
    if (rc) return rc;
    const uint64_t *d_aux = static_cast<const uint64_t *>(b->aux.p());
    if (split) {
        if ((rc = blm_rows32(b, total * static_cast<uint64_t>(nm), s, d_out))) return rc;
        if (own_offsets) std::copy(h_out_offsets, h_out_offsets + n_clips, aux.begin() + 2 * static_cast<size_t>(n_clips) + 1);
        h_out_offsets = nullptr;
        io &= 15;
    }
    HIP_TRY(hipMemcpyAsync(b->aux.p(), aux.data(), aux.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));    // pageable source: staged before the call returns
    BatchPlan pl;
    RaggedSlot *slot = nullptr;
    rc = plan_ragged(b->ragged, s, d_pcm, d_out, h_offsets, cols, h_out_offsets, n_clips, nm, kFbFPW, pl, slot);
    if (!rc) {
        FbankFastParams fp = blm_fast_params(b, pl.desc);
        fp.b.mel_major = 1;
        fp.b.sync_rounds = kNemoSync;
        fp.d_len = d_aux;
        fp.d_valid = d_aux + n_clips;
        rc = launch_nemo_mel(b, fp, io, s);
        if (!rc && b->cfg.normalize_per_feature && longest > 0) {
            // split: source rows at the plan's packed offsets in the scratch, destination rows at the caller's; otherwise in place
            const uint64_t *d_dst_off = own_offsets ? d_aux + 2 * static_cast<size_t>(n_clips) + 1 : pl.desc.d_out_off;
            const BlmNormRows rows{d_out, split ? vd_out : d_out, split ? out_dtype : MELSPEC_OUT_F32, n_clips, pl.desc.d_out_off, d_dst_off, pl.desc.d_frames, fp.d_valid};
            rc = launch_blm_norm_ragged(b, rows, longest, reinterpret_cast<unsigned *>(static_cast<uint64_t *>(b->aux.p()) + 2 * static_cast<size_t>(n_clips)), s);
        }
    }
    plan_ragged_done(slot, s);
    return rc;
}

int melspec_blm_compute_ragged_device(melspec_blm *b, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                      uint32_t n_clips, float *d_out, const uint64_t *h_out_offsets, void *stream) {
    return blm_ragged(b, d_pcm, h_offsets, h_lengths, n_clips, d_out, h_out_offsets, stream, 0);
}

// The same with the clip table in device memory: see include/melspec_hip.h.  The plan, d_len / d_valid and the normaliser's counter come
// from blm_plan_ragged_device_kernel; the launch is blm_ragged's, sized from the caller's two bounds -- n_units is the bound, the true count
// is at d_n_units, which every kernel route512 picks for a kLayout batch reads once per wave before its first round (batch_n_units in
// fbank512_wave_body.inc: one value for the whole workgroup, the planner having finished before the launch starts).
int melspec_blm_supports_desc(const melspec_blm *b) { return b && b->fast ? 1 : 0; }

int melspec_blm_compute_ragged_device_desc(melspec_blm *b, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths, uint32_t n_clips,
                                           float *d_out, const uint64_t *d_out_offsets, uint64_t max_total_columns, uint64_t max_clip_samples,
                                           uint32_t *d_rejected, void *stream) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (!b->fast) return fail(MELSPEC_ERR_UNSUPPORTED, "ragged batches need the fused kernel (n_fft = 512, win_length = 400)");
    if (n_clips == 0 || max_total_columns == 0 || max_clip_samples == 0) return MELSPEC_OK;
    if (!d_pcm || !d_out || !d_offsets || !d_lengths) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    const BlmDescGeom geom{static_cast<uint32_t>(b->cfg.n_fft), static_cast<uint32_t>(b->cfg.hop_length), static_cast<uint32_t>(b->cfg.pad_to), b->cfg.center ? 1u : 0u,
                           static_cast<uint32_t>(b->cfg.n_mels)};
    if (!blm_desc_bounds_ok(geom, max_total_columns, max_clip_samples))
        return fail(MELSPEC_ERR_UNSUPPORTED, "max_total_columns (< 2^40) or max_clip_samples (a row of < 2^31 columns) is too large for the device plan");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    BatchPlan pl;
    BlmDevicePlanAux aux{};
    int rc = blm_plan_ragged_device(b->dplan, s, d_pcm, d_out, d_offsets, d_lengths, d_out_offsets, n_clips, geom, max_total_columns, max_clip_samples, d_rejected, pl, aux);
    if (rc) return rc;
    FbankFastParams fp = blm_fast_params(b, pl.desc);
    fp.b.mel_major = 1;
    fp.b.sync_rounds = kNemoSync;
    fp.d_len = aux.d_len;
    fp.d_valid = aux.d_valid;
    if ((rc = launch_nemo_mel(b, fp, 0, s))) return rc;
    if (b->cfg.normalize_per_feature)
        rc = launch_blm_norm_ragged_desc(b, d_out, n_clips, pl.desc, aux, blm_desc_valid_frames(geom, max_clip_samples), s);
    return rc;
}

// ---- int16 PCM in / f16, bf16 rows out: see include/melspec_hip.h ----
int melspec_blm_supports_io(const melspec_blm *b, int pcm_dtype, int out_dtype) {
    if (!b || !io_pcm_known(pcm_dtype) || !io_out_known(out_dtype)) return 0;
    return (pcm_dtype == MELSPEC_PCM_F32 && out_dtype == MELSPEC_OUT_F32) || blm_io_ok(b) ? 1 : 0;
}

int melspec_blm_compute_uniform_device_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                          uint32_t n_clips, void *d_out, int out_dtype, void *stream) {
    int io, rc = blm_io_args(b, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    return blm_uniform(b, d_pcm, clip_stride, clip_len, n_clips, d_out, stream, io);
}

int melspec_blm_compute_ragged_device_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                         const uint64_t *h_lengths, uint32_t n_clips, void *d_out, int out_dtype,
                                         const uint64_t *h_out_offsets, void *stream) {
    int io, rc = blm_io_args(b, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    return blm_ragged(b, d_pcm, h_offsets, h_lengths, n_clips, d_out, h_out_offsets, stream, io);
}

// One clip from host memory (io = 0: the f32 call): the bytes of the caller's types cross the bus, the kernels convert.
static int blm_host(melspec_blm *b, const void *samples, size_t n_samples, void *out, size_t out_capacity_elems, size_t *rows, size_t *cols, int io) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (rows) *rows = static_cast<size_t>(b->cfg.n_mels);
    if (cols) *cols = 0;
    const uint64_t c = blm_padded(b, blm_valid_frames(b, n_samples));
    const int rc = host_one_clip(b->dev.device, b->h2d, b->d2h, b->stream, samples, n_samples * io_pcm_bytes(io & 15), out, out_capacity_elems,
                                 c * static_cast<uint64_t>(b->cfg.n_mels), io_out_bytes(io >> 4),
                                 [&](const void *d_in, void *d_out) { return blm_uniform(b, d_in, n_samples, n_samples, 1, d_out, b->stream, io); });
    if (!rc && cols) *cols = static_cast<size_t>(c);
    return rc;
}

int melspec_blm_compute_host_io(melspec_blm *b, const void *samples, int pcm_dtype, size_t n_samples, void *out, int out_dtype,
                                size_t out_capacity_elems, size_t *rows, size_t *cols) {
    int io, rc = blm_io_args(b, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    return blm_host(b, samples, n_samples, out, out_capacity_elems, rows, cols, io);
}

// ---- the split output: un-normalised rows + per-feature mean and 1 / (std + 1e-5), see include/melspec_hip.h ----
// the contexts whose kernels have the instantiations (blm_io_ok's condition), in the precision mode the context is in: the launch's LDS
// -- the mel kernel's, plus the f64 kernel's unit partials -- has to fit
static bool blm_stats_ok(const melspec_blm *b) {
    const Fused512Shape shape = blm_shape(b);
    return stats_ok(shape) && lds512(route512(shape, Batch512::kStats).run.lds, blm_lds(b)) <= kLdsLimit;
}

// the unsupported context's message, which names its geometry
static std::string blm_stats_unsupported(const melspec_blm *b) {
    return "the split output (rows + per-feature mean and 1 / std) is computed by the n_fft = 512 / win_length = 400 frontend with the 80- or 128-mel Slaney bank only; "
           "this context is n_fft = " + std::to_string(b->cfg.n_fft) + ", win_length = " + std::to_string(b->cfg.win_length) + ", n_mels = " +
           std::to_string(b->cfg.n_mels) + (b->fast ? " (another filterbank)" : "");
}

int melspec_blm_supports_split(const melspec_blm *b) { return b && blm_stats_ok(b) ? 1 : 0; }

int melspec_blm_compute_uniform_device_split(melspec_blm *b, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                             uint32_t n_clips, float *d_rows, float *d_mean, float *d_inv_std, void *stream) {
    const uint64_t valid = b ? blm_valid_frames(b, clip_len) : 0, cols = b ? blm_padded(b, valid) : 0;
    const BlmStatsArgs a = blm_stats_args(b != nullptr, b && blm_stats_ok(b), n_clips, cols, d_pcm, d_rows, d_mean, d_inv_std);
    if (a.verdict == kBlmStatsDone) return MELSPEC_OK;
    if (a.verdict == kBlmStatsFail) {
        if (a.msg) return fail(a.status, a.msg);
        g_last_error = blm_stats_unsupported(b);
        return a.status;
    }
    const int nm = b->cfg.n_mels;
    const Route512 r = route512(blm_shape(b), Batch512::kStats);
    BlmStatsPlan sp;
    if (!blm_stats_plan(cols, n_clips, nm, info_of(r.run.kernel).f32, sp)) return fail(MELSPEC_ERR_UNSUPPORTED, "the batch is too large for the split output's plan");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    int rc;
    if ((rc = b->stats.ensure(static_cast<size_t>(sp.part_bytes) + 16, s))) return rc;
    // the raw call's batch (blm_uniform with normalize_per_feature off), every clip's units rounded up to whole rounds of the workgroup
    BatchPlan pl = plan_uniform(d_pcm, d_rows, clip_stride, valid, n_clips, nm, kFbFPW, cols, true);
    pl.desc.units_per_clip = sp.units_per_clip;
    pl.desc.n_units = sp.n_units;
    FbankStatsParams q{};
    q.f = blm_fast_params(b, pl.desc);
    q.f.b.sync_rounds = kNemoSync;          // as the raw call: the f64 kernel's measured best, which is none (f32: the route's StagedRows)
    apply_route(r, q.f, b->f32);
    q.f.clip_len = static_cast<long long>(clip_len);
    q.d_part = static_cast<float2 *>(b->stats.p());
    q.blocks_per_clip = sp.blocks_per_clip;
    if ((rc = launch512(r.run, q, blm_lds(b), b->dev.cus, s))) return rc;
    BlmStatsFinishParams fq{};
    fq.part = q.d_part; fq.mean = d_mean; fq.inv_std = d_inv_std; fq.valid = valid;
    fq.n_clips = n_clips; fq.blocks_per_clip = sp.blocks_per_clip; fq.block_frames = sp.block_frames; fq.n_mels = nm;
    const uint64_t rows = static_cast<uint64_t>(n_clips) * nm;
    hipLaunchKernelGGL(blm_stats_finish_kernel, dim3(grid_for((rows + kBlmStatsFinishThreads - 1) / kBlmStatsFinishThreads, b->dev.cus, 8)), dim3(kBlmStatsFinishThreads), 0, s, fq);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// The ragged form: clip c = d_pcm[h_offsets[c] .. + h_lengths[c]) -> rows [n_mels][cols_c] at d_rows + h_rows_offsets[c] (NULL: packed in
// clip order) and mean / inv_std at [c][n_mels] -- the bits of the call above for that clip alone.  The batch is blm_ragged's raw batch
// with every clip's units rounded up to whole rounds of the workgroup (blm_stats_plan_ragged says what rests on that).
int melspec_blm_compute_ragged_device_split(melspec_blm *b, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                            float *d_rows, const uint64_t *h_rows_offsets, float *d_mean, float *d_inv_std, void *stream) {
    const bool ok = b && blm_stats_ok(b);
    // lengths, valid frames (the kernels' d_len / d_valid); the clips' columns
    std::vector<uint64_t> cols, aux;
    uint64_t most = 0;
    if (ok && n_clips && h_offsets && h_lengths) {
        cols.resize(n_clips);
        aux.resize(2 * static_cast<size_t>(n_clips));
        for (uint32_t i = 0; i < n_clips; ++i) {
            const uint64_t valid = blm_valid_frames(b, h_lengths[i]);
            cols[i] = blm_padded(b, valid);
            aux[i] = h_lengths[i];
            aux[n_clips + i] = valid;
            most = std::max(most, cols[i]);
        }
    }
    const BlmStatsArgs a = blm_stats_ragged_args(b != nullptr, ok, n_clips, h_offsets, h_lengths, most, d_pcm, d_rows, d_mean, d_inv_std);
    if (a.verdict == kBlmStatsDone) return MELSPEC_OK;
    if (a.verdict == kBlmStatsFail) {
        if (a.msg) return fail(a.status, a.msg);
        g_last_error = blm_stats_unsupported(b);
        return a.status;
    }
    const int nm = b->cfg.n_mels;
    const Route512 r = route512(blm_shape(b), Batch512::kStats);
    BlmStatsRaggedPlan sp;
    if (!blm_stats_plan_ragged(cols.data(), n_clips, nm, info_of(r.run.kernel).f32, sp)) return fail(MELSPEC_ERR_UNSUPPORTED, "the batch is too large for the split output's plan");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    int rc;
    if ((rc = b->stats.ensure(static_cast<size_t>(sp.part_bytes) + 16, s))) return rc;
    if ((rc = b->aux.ensure(aux.size() * sizeof(uint64_t), s))) return rc;
    const uint64_t *d_aux = static_cast<const uint64_t *>(b->aux.p());
    HIP_TRY(hipMemcpyAsync(b->aux.p(), aux.data(), aux.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));    // pageable source: staged before the call returns
    BatchPlan pl;
    RaggedSlot *slot = nullptr;
    rc = plan_ragged(b->ragged, s, d_pcm, d_rows, h_offsets, cols, h_rows_offsets, n_clips, nm, kFbFPW, pl, slot, false, sp.waves);
    // the kernels' waits count on whole rounds: a plan that disagrees with blm_stats_plan_ragged is not launched
    if (!rc && pl.desc.n_units != sp.n_units) rc = fail(MELSPEC_ERR_INTERNAL, "the split output's ragged plan and its batch plan disagree");
    if (!rc) {
        FbankStatsRaggedParams q{};
        q.f = blm_fast_params(b, pl.desc);
        q.f.b.mel_major = 1;
        q.f.b.sync_rounds = kNemoSync;          // as the raw call (f32: the route's StagedRows)
        apply_route(r, q.f, b->f32);
        q.f.d_len = d_aux;
        q.f.d_valid = d_aux + n_clips;
        q.d_part = static_cast<float2 *>(b->stats.p());
        rc = launch512(r.run, q, blm_lds(b), b->dev.cus, s);
        if (!rc) {
            BlmStatsFinishRaggedParams fq{};
            fq.part = q.d_part; fq.mean = d_mean; fq.inv_std = d_inv_std; fq.d_valid = q.f.d_valid; fq.d_unit_prefix = pl.desc.d_unit_prefix;
            fq.n_clips = n_clips; fq.waves = sp.waves; fq.block_frames = sp.block_frames; fq.n_mels = nm;
            const uint64_t rows = static_cast<uint64_t>(n_clips) * nm;
            hipLaunchKernelGGL(blm_stats_finish_ragged_kernel, dim3(grid_for((rows + kBlmStatsFinishThreads - 1) / kBlmStatsFinishThreads, b->dev.cus, 8)), dim3(kBlmStatsFinishThreads), 0, s, fq);
            if (hipGetLastError() != hipSuccess) rc = fail(MELSPEC_ERR_INTERNAL, "blm_stats_finish_ragged_kernel launch failed");
        }
    }
    plan_ragged_done(slot, s);
    return rc;
}

// One clip from host memory; the rows and the two statistics share the context's device-to-host buffer.
int melspec_blm_compute_host_split(melspec_blm *b, const float *samples, size_t n_samples, float *rows, size_t rows_capacity_floats,
                                   float *mean, float *inv_std, size_t *n_rows, size_t *n_cols) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (n_rows) *n_rows = static_cast<size_t>(b->cfg.n_mels);
    if (n_cols) *n_cols = 0;
    const uint64_t c = blm_padded(b, blm_valid_frames(b, n_samples));
    const uint64_t nm = static_cast<uint64_t>(b->cfg.n_mels), need = c * nm;
    if (blm_stats_ok(b) && c != 0) {        // (an unsupported context: the device call words the error)
        if (!samples || !rows) return fail(MELSPEC_ERR_INVALID_ARG, "samples/rows is NULL");
        if (!mean || !inv_std) return fail(MELSPEC_ERR_INVALID_ARG, "mean / inv_std is NULL");
        if (rows_capacity_floats < need) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
        HIP_TRY(hipSetDevice(b->dev.device));
        int rc;
        if ((rc = b->h2d.ensure(n_samples * sizeof(float)))) return rc;
        if ((rc = b->d2h.ensure((need + 2 * nm) * sizeof(float)))) return rc;
        HIP_TRY(hipMemcpyAsync(b->h2d.p, samples, n_samples * sizeof(float), hipMemcpyHostToDevice, b->stream));
    }
    float *d_rows = static_cast<float *>(b->d2h.p);
    const int rc = melspec_blm_compute_uniform_device_split(b, static_cast<const float *>(b->h2d.p), n_samples, n_samples, 1, d_rows, d_rows ? d_rows + need : nullptr,
                                                            d_rows ? d_rows + need + nm : nullptr, b->stream);
    if (rc || c == 0) return rc;
    HIP_TRY(hipMemcpyAsync(rows, d_rows, need * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(mean, d_rows + need, nm * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(inv_std, d_rows + need + nm, nm * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (n_cols) *n_cols = static_cast<size_t>(c);
    return MELSPEC_OK;
}

// ---- the split output with int16 PCM in / f16, bf16 rows out: see include/melspec_hip.h ----
// The f32 split calls above with the mel kernel's (sample, row) sibling (fbank512_stats_io_kernels.hpp): the same plans -- they count
// elements --, the same launch shape and LDS, the same partials scratch and finish kernels; b->rows32 is never touched.  (F32, F32) IS the
// call above.
int melspec_blm_supports_split_io(const melspec_blm *b, int pcm_dtype, int out_dtype) {
    return b && blm_split_io_pcm_known(pcm_dtype) && blm_split_io_out_known(out_dtype) && blm_stats_ok(b) ? 1 : 0;
}

// the verdict of an argument check as the call's status
static int blm_split_io_verdict(const melspec_blm *b, const BlmStatsArgs &a) {
    if (a.verdict != kBlmStatsFail) return MELSPEC_OK;
    if (a.msg) return fail(a.status, a.msg);
    g_last_error = blm_stats_unsupported(b);
    return a.status;
}

// one launch of the mel kernel of combination io behind the stats kernel of route r
static int launch_stats_io(const Launch512 &l, int io, const FbankStatsRaggedParams &q, const Lds512Sizes &z, int cus, hipStream_t s) {
    static std::atomic<uint64_t> attr_done[kBlmSplitIoKernels];          // one bit per device: function attributes are per device
    const int at = blm_split_io_slot(l.kernel, io);
    const FbankStatsIoKernel kernel = nemo_stats_io_kernel(l.kernel, io);
    if (at < 0 || !kernel) return fail(MELSPEC_ERR_INTERNAL, "launch_stats_io: the object has no kernel for this batch");
    if (int rc = allow_big_lds_once(attr_done[at], "hipFuncSetAttribute(fbank512_nemo_stats_io_kernel)", kernel)) return rc;
    hipLaunchKernelGGL(kernel, dim3(grid512(l, q.f.b.n_units, cus)), dim3(l.waves * 64), lds512(l.lds, z), s, q);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_blm_compute_uniform_device_split_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                                void *d_rows, int out_dtype, float *d_mean, float *d_inv_std, void *stream) {
    int io;
    const BlmStatsArgs codes = blm_split_io_codes(b != nullptr, pcm_dtype, out_dtype, io);
    if (codes.verdict == kBlmStatsFail) return blm_split_io_verdict(b, codes);
    if (io == 0) return melspec_blm_compute_uniform_device_split(b, static_cast<const float *>(d_pcm), clip_stride, clip_len, n_clips, static_cast<float *>(d_rows), d_mean, d_inv_std, stream);
    const uint64_t valid = blm_valid_frames(b, clip_len), cols = blm_padded(b, valid);
    const BlmStatsArgs a = blm_split_io_args(blm_stats_ok(b), n_clips, cols, d_pcm, d_rows, d_mean, d_inv_std, io);
    if (a.verdict != kBlmStatsGo) return blm_split_io_verdict(b, a);
    const int nm = b->cfg.n_mels;
    const Route512 r = route512(blm_shape(b), Batch512::kStats);
    BlmStatsPlan sp;
    if (!blm_stats_plan(cols, n_clips, nm, info_of(r.run.kernel).f32, sp)) return fail(MELSPEC_ERR_UNSUPPORTED, "the batch is too large for the split output's plan");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    int rc;
    if ((rc = b->stats.ensure(static_cast<size_t>(sp.part_bytes) + 16, s))) return rc;
    // the f32 split call's batch; the plan counts elements, the kernel reads the two pointers as its own types
    BatchPlan pl = plan_uniform(static_cast<const float *>(d_pcm), static_cast<float *>(d_rows), clip_stride, valid, n_clips, nm, kFbFPW, cols, true);
    pl.desc.units_per_clip = sp.units_per_clip;
    pl.desc.n_units = sp.n_units;
    FbankStatsRaggedParams q{};
    q.f = blm_fast_params(b, pl.desc);
    q.f.b.sync_rounds = kNemoSync;
    apply_route(r, q.f, b->f32);
    q.f.clip_len = static_cast<long long>(clip_len);
    q.d_part = static_cast<float2 *>(b->stats.p());          // [clip * blocks_per_clip + block][n_mels]: the layout blm_stats_finish_kernel reads
    if ((rc = launch_stats_io(r.run, io, q, blm_lds(b), b->dev.cus, s))) return rc;
    BlmStatsFinishParams fq{};
    fq.part = q.d_part; fq.mean = d_mean; fq.inv_std = d_inv_std; fq.valid = valid;
    fq.n_clips = n_clips; fq.blocks_per_clip = sp.blocks_per_clip; fq.block_frames = sp.block_frames; fq.n_mels = nm;
    const uint64_t rows = static_cast<uint64_t>(n_clips) * nm;
    hipLaunchKernelGGL(blm_stats_finish_kernel, dim3(grid_for((rows + kBlmStatsFinishThreads - 1) / kBlmStatsFinishThreads, b->dev.cus, 8)), dim3(kBlmStatsFinishThreads), 0, s, fq);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_blm_compute_ragged_device_split_io(melspec_blm *b, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                               void *d_rows, int out_dtype, const uint64_t *h_rows_offsets, float *d_mean, float *d_inv_std, void *stream) {
    int io;
    const BlmStatsArgs codes = blm_split_io_codes(b != nullptr, pcm_dtype, out_dtype, io);
    if (codes.verdict == kBlmStatsFail) return blm_split_io_verdict(b, codes);
    if (io == 0)
        return melspec_blm_compute_ragged_device_split(b, static_cast<const float *>(d_pcm), h_offsets, h_lengths, n_clips, static_cast<float *>(d_rows), h_rows_offsets, d_mean, d_inv_std, stream);
    const bool ok = blm_stats_ok(b);
    std::vector<uint64_t> cols, aux;          // the clips' columns; lengths, valid frames (the kernels' d_len / d_valid)
    uint64_t most = 0;
    if (ok && n_clips && h_offsets && h_lengths) {
        cols.resize(n_clips);
        aux.resize(2 * static_cast<size_t>(n_clips));
        for (uint32_t i = 0; i < n_clips; ++i) {
            const uint64_t valid = blm_valid_frames(b, h_lengths[i]);
            cols[i] = blm_padded(b, valid);
            aux[i] = h_lengths[i];
            aux[n_clips + i] = valid;
            most = std::max(most, cols[i]);
        }
    }
    const BlmStatsArgs a = blm_split_io_ragged_args(ok, n_clips, h_offsets, h_lengths, most, d_pcm, d_rows, d_mean, d_inv_std, io);
    if (a.verdict != kBlmStatsGo) return blm_split_io_verdict(b, a);
    const int nm = b->cfg.n_mels;
    const Route512 r = route512(blm_shape(b), Batch512::kStats);
    BlmStatsRaggedPlan sp;
    if (!blm_stats_plan_ragged(cols.data(), n_clips, nm, info_of(r.run.kernel).f32, sp)) return fail(MELSPEC_ERR_UNSUPPORTED, "the batch is too large for the split output's plan");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    int rc;
    if ((rc = b->stats.ensure(static_cast<size_t>(sp.part_bytes) + 16, s))) return rc;
    if ((rc = b->aux.ensure(aux.size() * sizeof(uint64_t), s))) return rc;
    const uint64_t *d_aux = static_cast<const uint64_t *>(b->aux.p());
    HIP_TRY(hipMemcpyAsync(b->aux.p(), aux.data(), aux.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));    // pageable source: staged before the call returns
    BatchPlan pl;
    RaggedSlot *slot = nullptr;
    rc = plan_ragged(b->ragged, s, static_cast<const float *>(d_pcm), static_cast<float *>(d_rows), h_offsets, cols, h_rows_offsets, n_clips, nm, kFbFPW, pl, slot, false, sp.waves);
    if (!rc && pl.desc.n_units != sp.n_units) rc = fail(MELSPEC_ERR_INTERNAL, "the split output's ragged plan and its batch plan disagree");
    if (!rc) {
        FbankStatsRaggedParams q{};
        q.f = blm_fast_params(b, pl.desc);
        q.f.b.mel_major = 1;
        q.f.b.sync_rounds = kNemoSync;
        apply_route(r, q.f, b->f32);
        q.f.d_len = d_aux;
        q.f.d_valid = d_aux + n_clips;
        q.d_part = static_cast<float2 *>(b->stats.p());
        rc = launch_stats_io(r.run, io, q, blm_lds(b), b->dev.cus, s);
        if (!rc) {
            BlmStatsFinishRaggedParams fq{};
            fq.part = q.d_part; fq.mean = d_mean; fq.inv_std = d_inv_std; fq.d_valid = q.f.d_valid; fq.d_unit_prefix = pl.desc.d_unit_prefix;
            fq.n_clips = n_clips; fq.waves = sp.waves; fq.block_frames = sp.block_frames; fq.n_mels = nm;
            const uint64_t rows = static_cast<uint64_t>(n_clips) * nm;
            hipLaunchKernelGGL(blm_stats_finish_ragged_kernel, dim3(grid_for((rows + kBlmStatsFinishThreads - 1) / kBlmStatsFinishThreads, b->dev.cus, 8)), dim3(kBlmStatsFinishThreads), 0, s, fq);
            if (hipGetLastError() != hipSuccess) rc = fail(MELSPEC_ERR_INTERNAL, "blm_stats_finish_ragged_kernel launch failed");
        }
    }
    plan_ragged_done(slot, s);
    return rc;
}

// One clip from host memory: the int16 bytes go up, the 16-bit rows and the two f32 vectors come back (the statistics behind the rows in
// the context's device-to-host buffer, at the next multiple of four bytes).
int melspec_blm_compute_host_split_io(melspec_blm *b, const void *samples, int pcm_dtype, size_t n_samples, void *rows, int out_dtype, size_t rows_capacity_elems,
                                      float *mean, float *inv_std, size_t *n_rows, size_t *n_cols) {
    int io;
    const BlmStatsArgs codes = blm_split_io_codes(b != nullptr, pcm_dtype, out_dtype, io);
    if (codes.verdict == kBlmStatsFail) return blm_split_io_verdict(b, codes);
    if (io == 0) return melspec_blm_compute_host_split(b, static_cast<const float *>(samples), n_samples, static_cast<float *>(rows), rows_capacity_elems, mean, inv_std, n_rows, n_cols);
    if (n_rows) *n_rows = static_cast<size_t>(b->cfg.n_mels);
    if (n_cols) *n_cols = 0;
    const uint64_t c = blm_padded(b, blm_valid_frames(b, n_samples));
    const uint64_t nm = static_cast<uint64_t>(b->cfg.n_mels), need = c * nm;
    const size_t in_bytes = blm_split_io_pcm_bytes(pcm_dtype), out_bytes = blm_split_io_out_bytes(out_dtype);
    const size_t stats_at = (static_cast<size_t>(need) * out_bytes + 3) & ~static_cast<size_t>(3);
    if (blm_stats_ok(b) && c != 0) {        // (an unsupported context: the device call words the error)
        if (!samples || !rows) return fail(MELSPEC_ERR_INVALID_ARG, "samples/rows is NULL");
        if (!mean || !inv_std) return fail(MELSPEC_ERR_INVALID_ARG, "mean / inv_std is NULL");
        if (rows_capacity_elems < need) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
        HIP_TRY(hipSetDevice(b->dev.device));
        int rc;
        if ((rc = b->h2d.ensure(n_samples * in_bytes))) return rc;
        if ((rc = b->d2h.ensure(stats_at + 2 * nm * sizeof(float)))) return rc;
        HIP_TRY(hipMemcpyAsync(b->h2d.p, samples, n_samples * in_bytes, hipMemcpyHostToDevice, b->stream));
    }
    char *d_rows = static_cast<char *>(b->d2h.p);
    float *d_stats = d_rows ? reinterpret_cast<float *>(d_rows + stats_at) : nullptr;
    const int rc = melspec_blm_compute_uniform_device_split_io(b, b->h2d.p, pcm_dtype, n_samples, n_samples, 1, d_rows, out_dtype, d_stats, d_stats ? d_stats + nm : nullptr, b->stream);
    if (rc || c == 0) return rc;
    HIP_TRY(hipMemcpyAsync(rows, d_rows, need * out_bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(mean, d_stats, nm * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipMemcpyAsync(inv_std, d_stats + nm, nm * sizeof(float), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (n_cols) *n_cols = static_cast<size_t>(c);
    return MELSPEC_OK;
}

int melspec_blm_release_scratch(melspec_blm *b) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    HIP_TRY(hipSetDevice(b->dev.device));
    HIP_TRY(hipStreamSynchronize(b->stream));
    if (int rc = b->aux.release_after(b->stream)) return rc;
    if (int rc = b->rows32.release_after(b->stream)) return rc;
    if (int rc = b->stats.release_after(b->stream)) return rc;
    if (b->dplan.used && b->dplan.last != b->stream) HIP_TRY(hipStreamSynchronize(b->dplan.last));
    b->pipe.release(); b->ragged.release(); b->dplan.release(); b->h2d.release(); b->d2h.release();
    return MELSPEC_OK;
}

int melspec_blm_synchronize(melspec_blm *b, void *stream) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    HIP_TRY(hipSetDevice(b->dev.device));
    HIP_TRY(hipStreamSynchronize(stream ? static_cast<hipStream_t>(stream) : b->stream));
    return MELSPEC_OK;
}

int melspec_blm_compute_host(melspec_blm *b, const float *samples, size_t n_samples, float *out, size_t out_capacity_floats,
                             size_t *rows, size_t *cols) {
    return blm_host(b, samples, n_samples, out, out_capacity_floats, rows, cols, 0);
}

// BatchLogMelSpectrogram::compute on many host clips in one call: clip i -> [n_mels][cols_i] floats at out + out_offsets[i] (NULL:
// packed), cols_i = melspec_blm_padded_frames(lengths[i]).  Whole clips in chunks through the host pipeline, one ragged launch per
// chunk (configurations on the generic kernel: one clip at a time).
int melspec_blm_compute_batch_host(melspec_blm *b, const float *samples, const uint64_t *offsets, const uint64_t *lengths, uint32_t n_clips,
                                   float *out, const uint64_t *out_offsets, size_t out_capacity_floats, uint64_t *total_columns) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "blm is NULL");
    if (total_columns) *total_columns = 0;
    const uint64_t nm = static_cast<uint64_t>(b->cfg.n_mels);
    std::vector<HostSeg> segs;
    uint64_t total;
    if (int rc = host_segments(samples, offsets, lengths, n_clips, out, out_offsets, out_capacity_floats, nm,
                               [b](uint64_t n) { return blm_padded(b, blm_valid_frames(b, n)); }, segs, total)) return rc;
    if (total_columns) *total_columns = total;
    if (total == 0) return MELSPEC_OK;
    HIP_TRY(hipSetDevice(b->dev.device));
    if (!b->fast) {
        for (const HostSeg &sg : segs) {
            const int rc = melspec_blm_compute_host(b, sg.src, static_cast<size_t>(sg.n), sg.dst, static_cast<size_t>(sg.frames * nm), nullptr, nullptr);
            if (rc) return rc;
        }
        return MELSPEC_OK;
    }
    return host_pipe_run(b->pipe, segs, b->cfg.n_mels, b->stream,
                         [b](const float *d_in, const uint64_t *offs, const uint64_t *lens, uint32_t n, float *d_out, const uint64_t *ooffs, hipStream_t s) {
                             return melspec_blm_compute_ragged_device(b, d_in, offs, lens, n, d_out, ooffs, s);
                         });
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// Kaldi fbank with int16 PCM in / f16, bf16 rows out (melspec_fbank_compute_*_io): see include/melspec_hip.h
// ------------------------------------------------------------------------------------
namespace {
bool fbank_io_ok(const melspec_fbank *fb) { return kaldi_io_ok(fbank_shape(fb)); }

// 0: go on (io = pcm_dtype | out_dtype << 4, 0 for (F32, F32)); otherwise the status to return
int fbank_io_args(const melspec_fbank *fb, int pcm_dtype, int out_dtype, int &io) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    if (int rc = io_dtypes(pcm_dtype, out_dtype, io)) return rc;
    if (io && !fbank_io_ok(fb)) {
        char geo[256];
        std::snprintf(geo, sizeof(geo), "sample_rate = %g, frame_length = %d samples, frame_shift = %d samples, num_mel_bins = %d, low_freq = %g, high_freq = %g",
                      fb->cfg.sample_rate, fb->frame_len, fb->frame_shift, fb->cfg.num_mel_bins, fb->cfg.low_freq, fb->cfg.high_freq);
        g_last_error = std::string("int16 PCM / f16, bf16 rows are computed by the fused fbank path with the compile-time 80-bin Kaldi bank only (16 kHz, "
                                   "400-sample frames, any frame shift, 80 bins, low_freq 20, high_freq Nyquist); this object is ") + geo +
                       (fb->use_generic ? " on the generic path (melspec_fbank_use_generic)" : (fb->fast ? " (another filterbank)" : ""));
        return MELSPEC_ERR_UNSUPPORTED;
    }
    return MELSPEC_OK;
}

}  // namespace

extern "C" {

int melspec_fbank_supports_io(const melspec_fbank *fb, int pcm_dtype, int out_dtype) {
    if (!fb || !io_pcm_known(pcm_dtype) || !io_out_known(out_dtype)) return 0;
    return (pcm_dtype == MELSPEC_PCM_F32 && out_dtype == MELSPEC_OUT_F32) || fbank_io_ok(fb) ? 1 : 0;
}

int melspec_fbank_compute_uniform_device_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len,
                                            uint32_t n_clips, void *d_out, int out_dtype, void *stream) {
    int io, rc = fbank_io_args(fb, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    return fbank_uniform(fb, d_pcm, clip_stride, clip_len, n_clips, d_out, stream, io);
}

int melspec_fbank_compute_ragged_device_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets,
                                           const uint64_t *h_lengths, uint32_t n_clips, void *d_out, int out_dtype,
                                           const uint64_t *h_out_offsets, void *stream) {
    int io, rc = fbank_io_args(fb, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    return fbank_ragged(fb, d_pcm, h_offsets, h_lengths, n_clips, d_out, h_out_offsets, stream, io);
}

// One clip from host memory (io = 0: the f32 call): the bytes of the caller's types cross the bus, the kernels convert.
static int fbank_host(melspec_fbank *fb, const void *samples, size_t n_samples, void *out, size_t out_capacity_elems, size_t *n_frames, int io) {
    if (!fb) return fail(MELSPEC_ERR_INVALID_ARG, "fbank is NULL");
    if (n_frames) *n_frames = 0;
    const uint64_t frames = fbank_frames(fb, n_samples);
    const int rc = host_one_clip(fb->dev.device, fb->h2d, fb->d2h, fb->stream, samples, n_samples * io_pcm_bytes(io & 15), out, out_capacity_elems,
                                 frames * static_cast<uint64_t>(fb->cfg.num_mel_bins), io_out_bytes(io >> 4),
                                 [&](const void *d_in, void *d_out) { return fbank_uniform(fb, d_in, n_samples, n_samples, 1, d_out, fb->stream, io); });
    if (!rc && n_frames) *n_frames = static_cast<size_t>(frames);
    return rc;
}

int melspec_fbank_compute_host(melspec_fbank *fb, const float *samples, size_t n_samples, float *out,
                               size_t out_capacity_floats, size_t *n_frames) {
    return fbank_host(fb, samples, n_samples, out, out_capacity_floats, n_frames, 0);
}

int melspec_fbank_compute_host_io(melspec_fbank *fb, const void *samples, int pcm_dtype, size_t n_samples,
                                  void *out, int out_dtype, size_t out_capacity_elems, size_t *n_frames) {
    int io, rc = fbank_io_args(fb, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    return fbank_host(fb, samples, n_samples, out, out_capacity_elems, n_frames, io);
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// Kaldi fbank, the split output with int16 PCM in / f16, bf16 rows out (melspec_fbank_compute_*_split_io): see include/melspec_hip.h.
// One pass: the workgroup-per-clip kernel's (sample, row) sibling (fbank512_kaldi_split_io_kernels.hpp) writes the caller's rows and the
// clips' means; fb->rows32 is never touched.  The plans are the f32 calls' -- they count elements --, the launch shape is the f32 clip
// kernel's (route512), the kernel comes from the side table of fbank512_kaldi_split_io.hip.  (F32, F32) IS the f32 split call.
// ------------------------------------------------------------------------------------
namespace {
bool fbank_split_io_supported(const melspec_fbank *fb) { return fbank_split_io_ok(fbank_shape(fb), fb->cfg.num_mel_bins); }       // (apply_cmn is part of the shape: cmn_power)

int fbank_split_io_verdict(const melspec_fbank *fb, const FbankSplitArgs &a) {
    if (a.verdict != kFbankSplitFail || a.msg) return fbank_split_verdict(a);
    char geo[320];
    std::snprintf(geo, sizeof(geo), "sample_rate = %g, frame_length = %d samples, frame_shift = %d samples, num_mel_bins = %d, low_freq = %g, high_freq = %g, use_power = %d",
                  fb->cfg.sample_rate, fb->frame_len, fb->frame_shift, fb->cfg.num_mel_bins, fb->cfg.low_freq, fb->cfg.high_freq, fb->cfg.use_power);
    g_last_error = std::string("the split output with int16 PCM / f16, bf16 rows is computed by the fused fbank path with the compile-time 80-bin Kaldi bank on power "
                               "spectra only (16 kHz, 400-sample frames, any frame shift, 80 bins, low_freq 20, high_freq Nyquist, use_power on); this object is ") + geo +
                   (fb->use_generic ? " on the generic path (melspec_fbank_use_generic)" : "");
    return a.status;
}

// one launch of the kernel of combination io over a uniform or a ragged-by-clip plan; fpc: frames per clip of a uniform batch
int launch_split_io(melspec_fbank *fb, bool ragged, int io, const BatchPlan &pl, uint64_t fpc, float *d_means, hipStream_t s) {
    static std::atomic<uint64_t> attr_done[kFbankSplitIoKernels];          // one bit per device: function attributes are per device
    const int nm = fb->cfg.num_mel_bins;
    const Launch512 l = route512(fbank_shape(fb), fbank_split_io_batch(ragged)).run;
    const Lds512Sizes z{fb->fast_lds, 0, nm};
    const int at = fbank_split_io_slot(ragged, io);
    const FbankClipSplitIoKernel kernel = kaldi_split_io_kernel(ragged, io);
    if (at < 0 || !kernel || !is_clip(l.kernel) || lds512(l.lds, z) > kLdsLimit) return fail(MELSPEC_ERR_INTERNAL, "launch_split_io: the object has no kernel for this batch");
    if (int rc = allow_big_lds_once(attr_done[at], "hipFuncSetAttribute(fbank512_clip_split_io_kernel)", kernel)) return rc;
    const FbankClipParams q{fbank_fast_params(fb, pl.desc), fpc, 0, d_means};
    hipLaunchKernelGGL(kernel, dim3(grid512(l, pl.desc.n_units, fb->dev.cus)), dim3(l.waves * 64), lds512(l.lds, z), s, q);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}
constexpr uint64_t kSplitIoMaxFrames = 1ull << 31;          // the kernel counts a clip's frames in 31 bits (clip_ragged_ok)
}  // namespace

extern "C" {

int melspec_fbank_supports_split_io(const melspec_fbank *fb, int pcm_dtype, int out_dtype) {
    return fb && fbank_split_io_pcm_known(pcm_dtype) && fbank_split_io_out_known(out_dtype) && fbank_split_io_supported(fb) ? 1 : 0;
}

int melspec_fbank_compute_uniform_device_split_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                                  void *d_rows, int out_dtype, float *d_means, void *stream) {
    int io;
    const FbankSplitArgs codes = fbank_split_io_codes(fb != nullptr, pcm_dtype, out_dtype, io);
    if (codes.verdict == kFbankSplitFail) return fbank_split_verdict(codes);
    if (io == 0) return melspec_fbank_compute_uniform_device_split(fb, static_cast<const float *>(d_pcm), clip_stride, clip_len, n_clips, static_cast<float *>(d_rows), d_means, stream);
    const uint64_t fpc = fbank_frames(fb, clip_len);
    const FbankSplitArgs a = fbank_split_args(fb->cfg.apply_cmn != 0, fbank_split_io_supported(fb), false, n_clips, nullptr, nullptr, fpc, d_pcm, d_rows, d_means, io);
    if (a.verdict == kFbankSplitZero) return fbank_split_zero_means(fb, d_means, n_clips, stream);
    if (a.verdict != kFbankSplitGo) return fbank_split_io_verdict(fb, a);
    if (fpc >= kSplitIoMaxFrames) return fail(MELSPEC_ERR_UNSUPPORTED, "a clip of 2^31 frames or more");
    HIP_TRY(hipSetDevice(fb->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fb->stream;
    // the f32 call's batch; the plan counts elements, the kernel reads the two pointers as its own types
    const BatchPlan pl = plan_uniform(static_cast<const float *>(d_pcm), static_cast<float *>(d_rows), clip_stride, fpc, n_clips, fb->cfg.num_mel_bins, kFbFPW);
    return launch_split_io(fb, false, io, pl, fpc, d_means, s);
}

int melspec_fbank_compute_ragged_device_split_io(melspec_fbank *fb, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                                 void *d_rows, int out_dtype, const uint64_t *h_rows_offsets, float *d_means, void *stream) {
    int io;
    const FbankSplitArgs codes = fbank_split_io_codes(fb != nullptr, pcm_dtype, out_dtype, io);
    if (codes.verdict == kFbankSplitFail) return fbank_split_verdict(codes);
    if (io == 0)
        return melspec_fbank_compute_ragged_device_split(fb, static_cast<const float *>(d_pcm), h_offsets, h_lengths, n_clips, static_cast<float *>(d_rows), h_rows_offsets, d_means, stream);
    const bool ok = fbank_split_io_supported(fb);
    std::vector<uint64_t> frames;
    uint64_t total = 0, longest = 0;
    bool frameless = false;
    if (ok && n_clips && h_offsets && h_lengths) {
        frames.resize(n_clips);
        for (uint32_t i = 0; i < n_clips; ++i) {
            frames[i] = fbank_frames(fb, h_lengths[i]);
            total += frames[i];
            longest = std::max(longest, frames[i]);
            frameless |= frames[i] == 0;
        }
    }
    const FbankSplitArgs a = fbank_split_args(fb->cfg.apply_cmn != 0, ok, true, n_clips, h_offsets, h_lengths, total, d_pcm, d_rows, d_means, io);
    if (a.verdict == kFbankSplitZero) return fbank_split_zero_means(fb, d_means, n_clips, stream);
    if (a.verdict != kFbankSplitGo) return fbank_split_io_verdict(fb, a);
    if (longest >= kSplitIoMaxFrames) return fail(MELSPEC_ERR_UNSUPPORTED, "a clip of 2^31 frames or more");
    HIP_TRY(hipSetDevice(fb->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : fb->stream;
    const int nm = fb->cfg.num_mel_bins;
    // the plan's order ends at the last clip with a frame: the kernel never sees the others, their mean slots are zeroed here
    if (frameless) HIP_TRY(hipMemsetAsync(d_means, 0, static_cast<size_t>(n_clips) * nm * sizeof(float), s));
    BatchPlan pl;
    RaggedSlot *slot = nullptr;
    int rc = plan_ragged(fb->ragged, s, static_cast<const float *>(d_pcm), static_cast<float *>(d_rows), h_offsets, frames, h_rows_offsets, n_clips, nm, kFbFPW, pl, slot, true);
    if (!rc) rc = launch_split_io(fb, true, io, pl, 0, d_means, s);
    plan_ragged_done(slot, s);
    return rc;
}

// One clip from host memory: the bytes of the caller's sample type go up, the rows of the caller's row type and the 80 means come back (the
// means behind the rows in the object's device-to-host buffer, at the next multiple of sixteen bytes).
int melspec_fbank_compute_host_split_io(melspec_fbank *fb, const void *samples, int pcm_dtype, size_t n_samples, void *rows, int out_dtype, size_t rows_capacity_elems,
                                        float *means, size_t *n_frames) {
    int io;
    const FbankSplitArgs codes = fbank_split_io_codes(fb != nullptr, pcm_dtype, out_dtype, io);
    if (codes.verdict == kFbankSplitFail) return fbank_split_verdict(codes);
    if (n_frames) *n_frames = 0;
    const uint64_t frames = fbank_frames(fb, n_samples);
    const uint64_t nm = static_cast<uint64_t>(fb->cfg.num_mel_bins), need = frames * nm;
    const size_t in_bytes = fbank_split_io_pcm_bytes(pcm_dtype), out_bytes = fbank_split_io_out_bytes(out_dtype);
    // the device call's checks in its order; of the host pointers only whether they are there ((F32, F32) runs on any object; host memory
    // needs no alignment, the staging buffers have it)
    static const float here = 0.0f;
    const FbankSplitArgs a = fbank_split_args(fb->cfg.apply_cmn != 0, io == 0 || fbank_split_io_supported(fb), false, 1, nullptr, nullptr, frames, samples ? &here : nullptr,
                                              rows ? &here : nullptr, means, 0);
    if (a.verdict == kFbankSplitZero) {
        std::fill(means, means + nm, 0.0f);
        return MELSPEC_OK;
    }
    if (a.verdict != kFbankSplitGo) return fbank_split_io_verdict(fb, a);
    if (rows_capacity_elems < need) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
    HIP_TRY(hipSetDevice(fb->dev.device));
    const size_t means_at = (static_cast<size_t>(need) * out_bytes + 15) & ~static_cast<size_t>(15);
    int rc;
    if ((rc = fb->h2d.ensure(n_samples * in_bytes))) return rc;
    if ((rc = fb->d2h.ensure(means_at + nm * sizeof(float)))) return rc;
    HIP_TRY(hipMemcpyAsync(fb->h2d.p, samples, n_samples * in_bytes, hipMemcpyHostToDevice, fb->stream));
    char *d_rows = static_cast<char *>(fb->d2h.p);
    float *d_means = reinterpret_cast<float *>(d_rows + means_at);
    if ((rc = melspec_fbank_compute_uniform_device_split_io(fb, fb->h2d.p, pcm_dtype, n_samples, n_samples, 1, d_rows, out_dtype, d_means, fb->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(rows, d_rows, need * out_bytes, hipMemcpyDeviceToHost, fb->stream));
    HIP_TRY(hipMemcpyAsync(means, d_means, nm * sizeof(float), hipMemcpyDeviceToHost, fb->stream));
    HIP_TRY(hipStreamSynchronize(fb->stream));
    if (n_frames) *n_frames = static_cast<size_t>(frames);
    return MELSPEC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// The stream banks of the two objects (melspec_fbank_stream_*, melspec_blm_stream_*): see include/melspec_hip.h.  The bank itself is
// written once, in stat_bank.hpp (StatBank<B> over stream_bank.hpp's core).  Here: the two sets of traits -- what a bank reads of its
// object, its planner (fbank_stream_plan.hpp / blm_stream_plan.hpp), its own tail (stat_bank_tail.hpp), its frame stage and the kernels
// behind it (fbank512_stream_kernels.hpp / fbank512_nemo_stream_kernels.hpp, stream_banks_io_kernels.hpp) -- and the ABI's forwards.
// ------------------------------------------------------------------------------------
namespace {
struct KaldiStream;
struct NemoStream;
using FbankStreamBank = StatBank<KaldiStream>;
using BlmStreamBank = StatBank<NemoStream>;

// Kaldi fbank: rows before CMN and their f64 column sums; the entries' tail is the clips' continues flags
struct KaldiStream {
    using Owner = melspec_fbank;
    using Geom = FbankStreamGeom;
    using Book = FbankStreamBook;            // total / emitted / pending per stream
    using Plan = FbankStreamPlan;
    static constexpr uint32_t kMagic = 0x4b53424du;
    static constexpr int kAccWords = 1, kStats = 1;          // sum; means
    static constexpr const char *kBankNull = "fbank stream bank is NULL", *kOwnerNull = "fbank is NULL", *kStatsDeviceNull = "d_means is NULL", *kStatsHostNull = "means is NULL",
                                *kChunksNull = "d_chunks is NULL: the chunks are at melspec_fbank_stream_input_ptr, which holds f32 (pcm_dtype must be MELSPEC_PCM_F32)";

    // the objects a bank can stand on: the fused 512-point path (every kernel of MS_K512_STREAM), frames that overlap or abut
    static bool ok(const Owner *fb) { return melspec_fbank_uses_fast_path(fb) && fb->frame_shift <= fb->frame_len; }
    static int supported(const Owner *fb) {
        if (ok(fb)) return MELSPEC_OK;
        char geo[256];
        std::snprintf(geo, sizeof(geo), "sample_rate = %g, frame_length = %d samples, frame_shift = %d samples, num_mel_bins = %d", fb->cfg.sample_rate,
                      fb->frame_len, fb->frame_shift, fb->cfg.num_mel_bins);
        g_last_error = std::string("the fbank stream bank runs on the fused fbank path (400-sample frames) with frame_shift <= frame_length; this object is ") + geo +
                       (fb->use_generic ? " on the generic path (melspec_fbank_use_generic)" : (fb->fast ? "" : " (generic path)"));
        return MELSPEC_ERR_UNSUPPORTED;
    }
    static Geom geometry(const Owner *fb, uint32_t n_streams, uint32_t max_chunk) {
        return fbank_stream_geometry(static_cast<uint32_t>(fb->frame_len), static_cast<uint32_t>(fb->frame_shift), static_cast<uint32_t>(fb->cfg.num_mel_bins), n_streams, max_chunk);
    }
    // the reference drops a stream's tail: nothing to finish, and no entry point says so
    static int plan(const Geom &g, Book &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool, Plan &pl, const char **err) {
        return fbank_stream_plan_push(g, bk, ids, lens, n, pl, err);
    }
    static void commit(const Geom &g, Book &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool) { fbank_stream_commit_push(g, bk, ids, lens, n); }
    static size_t frames_after(const Geom &g, const Book &bk, uint32_t id, uint32_t n_new) { return fbank_stream_frames_after(g, bk, id, n_new); }
    static std::vector<unsigned char> own_tail(const Plan &pl, uint32_t n) { return fbank_stream_own_tail(pl.continues.data(), n); }

    static int frames(const FbankStreamBank &st, const BatchPlan &bp, const void *d_tail, uint32_t, hipStream_t s) {
        melspec_fbank *fb = st.owner;
        FbankStreamParams q{};
        q.f = fbank_fast_params(fb, bp.desc);
        q.d_cont = static_cast<const uint32_t *>(d_tail);
        return launch512(route512(fbank_shape(fb), Batch512::kStream).run, q, Lds512Sizes{fb->fast_lds, 0, fb->cfg.num_mel_bins}, fb->dev.cus, s);
    }
    static hipError_t fold(const FbankStreamBank &st, const StreamEntry *d_e, const uint64_t *src_off, const float *rows, void *dst, int out_dtype, uint32_t n, hipStream_t s) {
        double *sums = static_cast<double *>(st.acc.p);
        unsigned long long *counts = static_cast<unsigned long long *>(st.counts.p);
        const int nm = static_cast<int>(st.geom.n_mels);
        if (src_off) return fbank_stream_sum_io_launch(FbankStreamSumIoParams{d_e, src_off, rows, dst, sums, counts, nm}, out_dtype, n, s);
        const FbankStreamSumParams sp{d_e, rows, sums, counts, nm};
        hipLaunchKernelGGL(fbank_stream_sum_kernel, dim3(n), dim3(kFbankStreamSumThreads), 0, s, sp);
        return hipGetLastError();
    }
    static void read_out(const FbankStreamBank &st, const uint32_t *d_ids, uint32_t n, float *const *out, hipStream_t s) {
        const FbankStreamMeanParams mp{d_ids, static_cast<const double *>(st.acc.p), static_cast<const unsigned long long *>(st.counts.p), out[0], n, static_cast<int>(st.geom.n_mels)};
        hipLaunchKernelGGL(fbank_stream_mean_kernel, st.stats_grid(n, kFbankStreamSumThreads), dim3(kFbankStreamSumThreads), 0, s, mp);
    }
};

// NeMo / Parakeet frontend: feature-major columns and their f64 Welford moments; the entries' tail is the clips' sample counts and,
// behind them, their window origins
struct NemoStream {
    using Owner = melspec_blm;               // with its precision mode
    using Geom = BlmStreamGeom;
    using Book = BlmStreamBook;              // total / emitted / ended per stream
    using Plan = BlmStreamPlan;
    static constexpr uint32_t kMagic = 0x4d4c424eu;
    static constexpr int kAccWords = 2, kStats = 2;          // mean, M2; mean, 1 / std
    static constexpr const char *kBankNull = "blm stream bank is NULL", *kOwnerNull = "blm is NULL", *kStatsDeviceNull = "d_mean / d_inv_std is NULL",
                                *kStatsHostNull = "mean / inv_std is NULL",
                                *kChunksNull = "d_chunks is NULL: the chunks are at melspec_blm_stream_input_ptr, which holds f32 (pcm_dtype must be MELSPEC_PCM_F32)";

    // the contexts a bank can stand on: the fused 512-point path (every kernel of MS_K512_NEMO_STREAM)
    static bool ok(const Owner *b) { return b->fast; }
    static int supported(const Owner *b) {
        if (ok(b)) return MELSPEC_OK;
        g_last_error = "the log-mel stream bank runs on the fused kernels (n_fft = 512, win_length = 400); this context is n_fft = " + std::to_string(b->cfg.n_fft) +
                       ", win_length = " + std::to_string(b->cfg.win_length) + ", hop_length = " + std::to_string(b->cfg.hop_length) + ", n_mels = " + std::to_string(b->cfg.n_mels) +
                       (b->cfg.n_fft == 512 && b->cfg.win_length == 400 ? " (a filterbank the fused kernels do not hold)" : "");
        return MELSPEC_ERR_UNSUPPORTED;
    }
    static Geom geometry(const Owner *b, uint32_t n_streams, uint32_t max_chunk) {
        return blm_stream_geometry(static_cast<uint32_t>(b->cfg.hop_length), b->cfg.center != 0, static_cast<uint32_t>(b->cfg.n_mels), n_streams, max_chunk);
    }
    static int plan(const Geom &g, Book &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool finish, Plan &pl, const char **err) {
        return blm_stream_plan_push(g, bk, ids, lens, n, finish, pl, err);
    }
    static void commit(const Geom &g, Book &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool finish) { blm_stream_commit_push(g, bk, ids, lens, n, finish); }
    static size_t frames_after(const Geom &g, const Book &bk, uint32_t id, uint32_t n_new) { return blm_stream_frames_after(g, bk, id, n_new); }
    static std::vector<unsigned char> own_tail(const Plan &pl, uint32_t n) { return blm_stream_own_tail(pl.len.data(), pl.org0.data(), n); }

    // the ragged batch of blm_ragged over the state: feature-major rows as wide as the entry's frames, every one of them valid
    static int frames(const BlmStreamBank &st, const BatchPlan &bp, const void *d_tail, uint32_t n, hipStream_t s) {
        melspec_blm *b = st.owner;
        FbankNemoStreamParams q{};
        q.f = blm_fast_params(b, bp.desc);
        q.f.b.mel_major = 1;
        q.f.b.sync_rounds = kNemoSync;
        q.f.d_len = static_cast<const uint64_t *>(d_tail);
        q.f.d_valid = bp.desc.d_frames;
        q.d_org0 = reinterpret_cast<const int *>(static_cast<const char *>(d_tail) + blm_stream_org0_at(n));
        const Route512 r = route512(blm_shape(b), Batch512::kLayout);      // the kernel a batch of the context runs on now; its stream form
        apply_route(r, q.f, b->f32);
        return launch512(r.run, q, blm_lds(b), b->dev.cus, s);
    }
    static hipError_t fold(const BlmStreamBank &st, const StreamEntry *d_e, const uint64_t *src_off, const float *rows, void *dst, int out_dtype, uint32_t n, hipStream_t s) {
        double *moments = static_cast<double *>(st.acc.p);
        unsigned long long *counts = static_cast<unsigned long long *>(st.counts.p);
        const int nm = static_cast<int>(st.geom.n_mels);
        if (src_off) return blm_stream_stats_io_launch(BlmStreamStatsIoParams{d_e, src_off, rows, dst, moments, counts, nm, 0}, out_dtype, n, s);
        const BlmStreamStatsParams sp{d_e, rows, moments, counts, nm};
        hipLaunchKernelGGL(blm_stream_stats_kernel, dim3(n), dim3(kBlmStreamStatsThreads), 0, s, sp);
        return hipGetLastError();
    }
    static void read_out(const BlmStreamBank &st, const uint32_t *d_ids, uint32_t n, float *const *out, hipStream_t s) {
        const BlmStreamMomentsParams mp{d_ids, static_cast<const double *>(st.acc.p), static_cast<const unsigned long long *>(st.counts.p), out[0], out[1], n, static_cast<int>(st.geom.n_mels)};
        hipLaunchKernelGGL(blm_stream_moments_kernel, st.stats_grid(n, kBlmStreamStatsThreads), dim3(kBlmStreamStatsThreads), 0, s, mp);
    }
};
}  // namespace

extern "C" {

int melspec_fbank_stream_create(void **out, melspec_fbank *fb, uint32_t n_streams, uint32_t max_chunk) { return FbankStreamBank::create(out, fb, n_streams, max_chunk); }
void melspec_fbank_stream_destroy(void *h) { FbankStreamBank::destroy(h); }
int melspec_fbank_stream_reset(void *h, const uint32_t *ids, uint32_t n) { return FbankStreamBank::reset(h, ids, n); }
size_t melspec_fbank_stream_frames_after(const void *h, uint32_t id, uint32_t n_new) { return FbankStreamBank::frames_after(h, id, n_new); }
float *melspec_fbank_stream_input_ptr(void *h, uint32_t id) { return FbankStreamBank::input_ptr(h, id); }
int melspec_fbank_stream_supports_io(const void *h, int pcm_dtype, int out_dtype) { return FbankStreamBank::supports_io(h, pcm_dtype, out_dtype); }

int melspec_fbank_stream_push_host(void *h, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n, float *out,
                                   size_t out_capacity_floats, uint32_t *frames_out) {
    return FbankStreamBank::push_host(h, ids, samples, pcm_dtype, lens, n, false, out, MELSPEC_OUT_F32, out_capacity_floats, frames_out);
}
int melspec_fbank_stream_push_host_io(void *h, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n, void *out,
                                      int out_dtype, size_t out_capacity_elems, uint32_t *frames_out) {
    return FbankStreamBank::push_host(h, ids, samples, pcm_dtype, lens, n, false, out, out_dtype, out_capacity_elems, frames_out);
}
int melspec_fbank_stream_push_device(void *h, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets, const uint32_t *lens,
                                     uint32_t n, float *d_out, const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream) {
    return FbankStreamBank::push_device(h, ids, d_chunks, pcm_dtype, h_src_offsets, lens, n, false, d_out, MELSPEC_OUT_F32, h_out_offsets, frames_out, stream);
}
int melspec_fbank_stream_push_device_io(void *h, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets, const uint32_t *lens,
                                        uint32_t n, void *d_out, int out_dtype, const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream) {
    return FbankStreamBank::push_device(h, ids, d_chunks, pcm_dtype, h_src_offsets, lens, n, false, d_out, out_dtype, h_out_offsets, frames_out, stream);
}

int melspec_fbank_stream_stats_device(void *h, const uint32_t *ids, uint32_t n, float *d_means, uint64_t *h_counts, void *stream) {
    float *const out[] = {d_means};
    return FbankStreamBank::stats_device(h, ids, n, out, h_counts, stream);
}
int melspec_fbank_stream_stats_host(void *h, const uint32_t *ids, uint32_t n, float *means, uint64_t *counts) {
    float *const out[] = {means};
    return FbankStreamBank::stats_host(h, ids, n, out, counts);
}

int melspec_blm_stream_create(void **out, melspec_blm *b, uint32_t n_streams, uint32_t max_chunk) { return BlmStreamBank::create(out, b, n_streams, max_chunk); }
void melspec_blm_stream_destroy(void *h) { BlmStreamBank::destroy(h); }
int melspec_blm_stream_reset(void *h, const uint32_t *ids, uint32_t n) { return BlmStreamBank::reset(h, ids, n); }
size_t melspec_blm_stream_frames_after(const void *h, uint32_t id, uint32_t n_new) { return BlmStreamBank::frames_after(h, id, n_new); }
size_t melspec_blm_stream_finish_frames(const void *h, uint32_t id) {
    const BlmStreamBank *st = BlmStreamBank::of(h);
    return st && id < st->geom.n_streams ? blm_stream_finish_frames(st->geom, st->book, id) : 0;
}
float *melspec_blm_stream_input_ptr(void *h, uint32_t id) { return BlmStreamBank::input_ptr(h, id); }
int melspec_blm_stream_supports_io(const void *h, int pcm_dtype, int out_dtype) { return BlmStreamBank::supports_io(h, pcm_dtype, out_dtype); }

int melspec_blm_stream_push_host(void *h, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n, float *out,
                                 size_t out_capacity_floats, uint32_t *frames_out) {
    return BlmStreamBank::push_host(h, ids, samples, pcm_dtype, lens, n, false, out, MELSPEC_OUT_F32, out_capacity_floats, frames_out);
}
int melspec_blm_stream_push_host_io(void *h, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n, void *out, int out_dtype,
                                    size_t out_capacity_elems, uint32_t *frames_out) {
    return BlmStreamBank::push_host(h, ids, samples, pcm_dtype, lens, n, false, out, out_dtype, out_capacity_elems, frames_out);
}
int melspec_blm_stream_push_device(void *h, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets, const uint32_t *lens,
                                   uint32_t n, float *d_out, const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream) {
    return BlmStreamBank::push_device(h, ids, d_chunks, pcm_dtype, h_src_offsets, lens, n, false, d_out, MELSPEC_OUT_F32, h_out_offsets, frames_out, stream);
}
int melspec_blm_stream_push_device_io(void *h, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets, const uint32_t *lens,
                                      uint32_t n, void *d_out, int out_dtype, const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream) {
    return BlmStreamBank::push_device(h, ids, d_chunks, pcm_dtype, h_src_offsets, lens, n, false, d_out, out_dtype, h_out_offsets, frames_out, stream);
}

// a finish is a push of no samples with the planner's finish flag
int melspec_blm_stream_finish_host(void *h, const uint32_t *ids, uint32_t n, float *out, size_t out_capacity_floats, uint32_t *frames_out) {
    return BlmStreamBank::push_host(h, ids, nullptr, MELSPEC_PCM_F32, nullptr, n, true, out, MELSPEC_OUT_F32, out_capacity_floats, frames_out);
}
int melspec_blm_stream_finish_host_io(void *h, const uint32_t *ids, uint32_t n, void *out, int out_dtype, size_t out_capacity_elems, uint32_t *frames_out) {
    return BlmStreamBank::push_host(h, ids, nullptr, MELSPEC_PCM_F32, nullptr, n, true, out, out_dtype, out_capacity_elems, frames_out);
}
int melspec_blm_stream_finish_device(void *h, const uint32_t *ids, uint32_t n, float *d_out, const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream) {
    return BlmStreamBank::push_device(h, ids, nullptr, MELSPEC_PCM_F32, nullptr, nullptr, n, true, d_out, MELSPEC_OUT_F32, h_out_offsets, frames_out, stream);
}
int melspec_blm_stream_finish_device_io(void *h, const uint32_t *ids, uint32_t n, void *d_out, int out_dtype, const uint64_t *h_out_offsets, uint32_t *frames_out,
                                        void *stream) {
    return BlmStreamBank::push_device(h, ids, nullptr, MELSPEC_PCM_F32, nullptr, nullptr, n, true, d_out, out_dtype, h_out_offsets, frames_out, stream);
}

int melspec_blm_stream_stats_device(void *h, const uint32_t *ids, uint32_t n, float *d_mean, float *d_inv_std, uint64_t *h_counts, void *stream) {
    float *const out[] = {d_mean, d_inv_std};
    return BlmStreamBank::stats_device(h, ids, n, out, h_counts, stream);
}
int melspec_blm_stream_stats_host(void *h, const uint32_t *ids, uint32_t n, float *mean, float *inv_std, uint64_t *counts) {
    float *const out[] = {mean, inv_std};
    return BlmStreamBank::stats_host(h, ids, n, out, counts);
}

}  // extern "C"

