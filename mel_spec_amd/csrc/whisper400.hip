// whisper400.hip -- launchers of the fused n_fft = 400 kernels (whisper400_kernels.hpp): launch_ctx runs a batch of a melspec_ctx on the
// kernels its route names (ctx_route.hpp) -- f32 with the precision guard and the vote, or f64 -- and launch_stft exports the spectrum (row a3).
#include "host_common.hpp"
#include "whisper400_io_kernels.hpp"
namespace melspec {
// emitted by melspec_runs.hip (compiled with its own scheduling strategy; see there)
extern template __global__ void whisper400_six_runs_kernel<kSixMaxSlots, LensSix80>(const FastParams);
extern template __global__ void whisper400_wave_runs_kernel<8, LensI80>(const FastParams);
extern template __global__ void whisper400_wave_runs_kernel<12, LensI128>(const FastParams);
extern template __global__ void whisper400_six_wide_runs_kernel<kSixWideSlots, LensSix128>(const FastParams);
// emitted by melspec_io_runs.hip / melspec_io64.hip: int16 PCM in and / or f16, bf16 rows out
#define MS_IO_EXTERN(In, Out)                                                                                                  \
    extern template __global__ void whisper400_six_runs_io_kernel<kSixMaxSlots, LensSix80, In, Out>(const FastParams);        \
    extern template __global__ void whisper400_six_wide_runs_io_kernel<kSixWideSlots, LensSix128, In, Out>(const FastParams); \
    extern template __global__ void whisper400_six64_io_kernel<kSixMaxSlots, LensSix80, In, Out>(const Six64Params);          \
    extern template __global__ void whisper400_six64_io_kernel<kSixWideSlots, LensSix128, In, Out>(const Six64Params);
MS_IO_COMBOS(MS_IO_EXTERN)
#undef MS_IO_EXTERN
}  // namespace melspec

namespace melspec {
namespace host {

// MELSPEC_PRECISION_AUTO: take in what the finished launches published (reporting only: melspec_auto_state)
void auto_poll(melspec_ctx *c) {
    FixState &fx = c->fix;
    if (!fx.host) return;
    const volatile unsigned long long *h = fx.host;
    const unsigned long long a = h[0], b = h[1];
    const uint32_t seq = static_cast<uint32_t>(a >> kStatShift);
    if (seq != static_cast<uint32_t>(b >> kStatShift) || seq == fx.seen_seq) return;     // a launch is publishing right now, or nothing new
    fx.seen_seq = seq;
    const unsigned long long tripped = a & kStatMask, frames = b & kStatMask & ~kStatFromGated;
    fx.heavy = (b & kStatFromGated) != 0;
    if (frames < kAutoMinFrames) return;
    fx.fraction = static_cast<double>(tripped) / static_cast<double>(frames);
}

int auto_sink(melspec_ctx *c, const BatchDesc &desc, hipStream_t stream, bool with_vote, FixSink &sink) {
    FixState &fx = c->fix;
    if (fx.used && fx.last_stream != stream) HIP_TRY(hipStreamSynchronize(fx.last_stream));
    const size_t need = (static_cast<size_t>(desc.n_units) + 65536) * sizeof(uint64_t);      // one note per unit + a round of slack
    if (need > fx.list.cap) {
        if (fx.used) HIP_TRY(hipStreamSynchronize(fx.last_stream));       // a launch in flight may still write the old list
        int rc = fx.list.ensure(need);
        if (rc) return rc;
    }
    sink.tab = static_cast<const double *>(fx.tab.p);
    sink.list = static_cast<uint64_t *>(fx.list.p);
    if (!fx.host) {
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&fx.host), 64, hipHostMallocMapped | hipHostMallocCoherent));
        std::memset(fx.host, 0, 64);
    }
    fx.used = true; fx.last_stream = stream;
    sink.count = static_cast<unsigned long long *>(fx.count.p);
    sink.acc = sink.count + 1;
    sink.host = fx.host;
    if (with_vote) {
        sink.vote = sink.count + 2;
        sink.decision = static_cast<unsigned *>(fx.verdicts.p);
    }
    return MELSPEC_OK;
}

// the launch-specific part of a guarded launch's statistics sink (the grid is only known where the launch is made)
FixSink sink_armed(melspec_ctx *c, FixSink sink, const BatchDesc &desc, unsigned grid) {
    if (!sink.acc) return sink;
    sink.frames = desc.stat_frames ? desc.stat_frames
                : desc.d_unit_prefix == nullptr ? static_cast<uint64_t>(desc.n_clips) * desc.frames_per_clip
                                                : desc.n_units * static_cast<uint64_t>(desc.frames_per_unit);   // device-planned ragged: upper bound
    sink.n_groups = grid;
    sink.seq = (c->fix.seq = (c->fix.seq + 1) & 0xffffffu) ? c->fix.seq : (c->fix.seq = 1);      // never 0: the host's "nothing seen yet"
    return sink;
}

// The f64 five-frame kernel on the whole batch: MELSPEC_PRECISION_F64 (the plan is its own, kFPW frames per unit), or -- gate != nullptr --
// AUTO's second launch, which runs only when the f32 launch in front of it voted "heavy" and walks THAT launch's plan (plain batches).
// k: one of F64Kernel::kPrecise*
int launch_precise(melspec_ctx *c, const BatchDesc &desc, const FixSink &stat, hipStream_t stream, F64Kernel k, const unsigned *gate, unsigned gate_value) {
    typedef void (*Kernel)(const PreciseParams);
#define MS_PRECISE(NSLOTS, Lens) {&whisper400_precise_kernel<NSLOTS, Lens, 0>, &whisper400_precise_kernel<NSLOTS, Lens, 1>, &whisper400_precise_kernel<NSLOTS, Lens, 2>}
    static const Kernel table[4][3] = {MS_PRECISE(8, LensI80), MS_PRECISE(8, LensRuntime), MS_PRECISE(12, LensI128), MS_PRECISE(12, LensRuntime)};     // [.][layout, runs, gated]
#undef MS_PRECISE
    static std::atomic<uint64_t> attr_done[4];          // one bit per device: function attributes are per device
    const int i = static_cast<int>(k) - static_cast<int>(F64Kernel::kPrecise8I80);
    if (i < 0 || i > 3) return fail(MELSPEC_ERR_INTERNAL, "launch_precise: not a whisper400_precise_kernel");
    if (int rc = allow_big_lds_once(attr_done[i], "hipFuncSetAttribute(whisper400_precise_kernel)", table[i][0], table[i][1], table[i][2])) return rc;
    const bool layout = is_layout(desc);
    const bool walk = gate && !layout;      // gated layouts come with a plan of their own
    const uint64_t steps = walk ? (desc.n_units * static_cast<uint64_t>(desc.frames_per_unit) + kFPW - 1) / kFPW : desc.n_units;
    const uint64_t blocks = (steps + kPreciseWaves - 1) / kPreciseWaves;
    static const int per_cu = lab_int("MELSPEC_PRECISE_GRID_PER_CU", 1, 1, 4096);   // one workgroup is resident per CU
    const unsigned grid = grid_for_xcd(blocks, c->dev.cus, per_cu);
    FixSink armed = sink_armed(c, stat, desc, grid);
    if (gate) armed.frames |= kStatFromGated;
    PreciseParams pp{};
    pp.b = desc;
    pp.stat = armed;
    pp.d_blob = static_cast<const uint32_t *>(c->d_blob64.p);
    pp.blob_words = static_cast<int>(c->pt.blob.size());
    pp.mel_off_words = c->pt.mel_off_words;
    pp.hop = c->hop_size;
    pp.n_mels = c->n_mels;
    pp.slots = c->ft.slots;
    pp.gate = gate; pp.gate_value = gate_value; pp.plan_fpu = desc.frames_per_unit;
    hipLaunchKernelGGL(table[i][layout ? 0 : gate ? 2 : 1], dim3(grid), dim3(kPreciseWaves * 64), c->precise_lds, stream, pp);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// The f64 six-frame kernel k on a batch planned in six-frame units: MELSPEC_PRECISION_F64, or -- gate != nullptr -- AUTO's second launch
// over the plan of the f32 launch in front of it
typedef void (*Six64Kernel)(const Six64Params);
int launch_six64(melspec_ctx *c, const BatchDesc &desc, const FixSink &stat, hipStream_t stream, Six64Kernel k, const unsigned *gate, unsigned gate_value) {
    const uint64_t blocks = (desc.n_units + kSix64Waves - 1) / kSix64Waves;
    static const int per_cu = lab_int("MELSPEC_SIX64_GRID_PER_CU", 1, 1, 4096);   // one 12-wave workgroup is resident per CU
    const unsigned grid = grid_for_xcd(blocks, c->dev.cus, per_cu);
    FixSink armed = sink_armed(c, stat, desc, grid);
    if (gate) armed.frames |= kStatFromGated;
    Six64Params pp{};
    pp.b = desc;
    pp.stat = armed;
    pp.d_blob = static_cast<const uint32_t *>(c->d_blob64x.p);
    pp.blob_words = static_cast<int>(c->t64.blob.size());
    pp.mel_off_words = c->t64.mel_off_words;
    pp.hop = c->hop_size;
    pp.n_mels = c->n_mels;
    pp.slots = c->ft6.slots;
    pp.gate = gate; pp.gate_value = gate_value;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kSix64Waves * 64), c->lds64x, stream, pp);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// the kernel of F64Kernel::kSix64* (the layout form exists for the compile-time banks of up to 80 mels only), allowed the whole LDS
int six64_kernel(F64Kernel k, Six64Kernel &kernel) {
    struct Pair { Six64Kernel plain, layout; };
    static const Pair table[5] = {{&whisper400_six64_kernel<kSixMaxSlots, LensSix80>, &whisper400_six64_layout_kernel<kSixMaxSlots, LensSix80>},
                                  {&whisper400_six64_kernel<kSixMaxSlots, LensSix64>, &whisper400_six64_layout_kernel<kSixMaxSlots, LensSix64>},
                                  {&whisper400_six64_kernel<kSixMaxSlots, LensSix40>, &whisper400_six64_layout_kernel<kSixMaxSlots, LensSix40>},
                                  {&whisper400_six64_kernel<kSixMaxSlots, LensRuntime>, nullptr},
                                  {&whisper400_six64_kernel<kSixWideSlots, LensSix128>, nullptr}};
    static std::atomic<uint64_t> attr_done[5];
    const bool layout = is_six64_layout(k);
    const int i = static_cast<int>(k) - static_cast<int>(layout ? F64Kernel::kSix64LayoutL80 : F64Kernel::kSix64L80);
    if (!is_six64(k) || i < 0 || i > 4) return fail(MELSPEC_ERR_INTERNAL, "six64_kernel: not a whisper400_six64_kernel");
    const Pair &p = table[i];
    kernel = layout ? p.layout : p.plain;
    return allow_big_lds_once(attr_done[i], "hipFuncSetAttribute(whisper400_six64_kernel)", p.plain, p.layout ? p.layout : p.plain);
}

// ---- int16 PCM in / f16, bf16 rows out (melspec_compute_*_io): the kernels of a (sample, row) combination -----------------------------------
// They stand in for the f32 / f64 six-frame kernels of a plain batch in the same launches: same grid, same run per wave, same vote sample,
// same sink -- AUTO gives the same bits and the same statistics as the f32 call on the converted batch.
typedef void (*FastKernel)(const FastParams);
struct IoKernels {
    FastKernel runs80, runs128;
    Six64Kernel f64_80, f64_128;
};
template <class In, class Out>
IoKernels io_kernels_of() {
    return IoKernels{&whisper400_six_runs_io_kernel<kSixMaxSlots, LensSix80, In, Out>, &whisper400_six_wide_runs_io_kernel<kSixWideSlots, LensSix128, In, Out>,
                     &whisper400_six64_io_kernel<kSixMaxSlots, LensSix80, In, Out>, &whisper400_six64_io_kernel<kSixWideSlots, LensSix128, In, Out>};
}
// io = pcm_dtype | out_dtype << 4, not (F32, F32); the kernels are allowed the whole LDS once per device and combination
int io_kernels(int io, const IoKernels *&k) {
    static const IoKernels table[2][3] = {{IoKernels{}, io_kernels_of<float, io_f16>(), io_kernels_of<float, io_bf16>()},
                                          {io_kernels_of<io_s16, float>(), io_kernels_of<io_s16, io_f16>(), io_kernels_of<io_s16, io_bf16>()}};
    static std::atomic<uint64_t> attr_done[2][3];
    const int pcm = io & 15, out = io >> 4;
    if (pcm < 0 || pcm > 1 || out < 0 || out > 2 || io == 0) return fail(MELSPEC_ERR_INTERNAL, "io_kernels: no such combination");
    k = &table[pcm][out];
    return allow_big_lds_once(attr_done[pcm][out], "hipFuncSetAttribute(whisper400 _io kernels)", k->runs80, k->runs128, k->f64_80, k->f64_128);
}

// ---- the f32 kernels: every one takes FastParams -----------------------------------------------------------------------------------------
// Plain batches, uniform and ragged, take the run-per-wave member (no division per unit, the clip record in scalar registers, a wave
// re-reads its own frame-tail halo: cfg2 0.3105 -> 0.3055 ms, 8192 x 30 s 7.55 -> 7.42 ms against the round-robin deal); the layouts
// deal their units round-robin.
struct FastFamily {
    FastKernel runs, layout;
    int waves;            // per workgroup
    int per_cu;           // workgroups per CU the grid is cut to
    int bank;             // the context's tables: 0 five-frame, 1 six-frame, 2 six-frame with fifteen slots
    std::atomic<uint64_t> done;
};
FastFamily &fast_family(F32Kernel k) {
    static const int six_per_cu = lab_int("MELSPEC_SIX_GRID_PER_CU", 1, 1, 4096);     // one workgroup per CU
    // two workgroups are resident per CU; 4 per CU measured best (8192 x 15..45 s x 128 mels: 9.17 vs 9.50 ms)
    static const int wave_per_cu = lab_int("MELSPEC_GRID_PER_CU", 4, 1, 64);
#define MS_FAMILY(runs, layout, ...) {&runs<__VA_ARGS__>, &layout<__VA_ARGS__>
    static FastFamily table[static_cast<int>(F32Kernel::kCount)] = {
        {},
        MS_FAMILY(whisper400_six_runs_kernel, whisper400_six_kernel, kSixMaxSlots, LensSix80), kSixWaves, six_per_cu, 1},
        MS_FAMILY(whisper400_six_runs_kernel, whisper400_six_kernel, kSixMaxSlots, LensRuntime), kSixWaves, six_per_cu, 1},
        MS_FAMILY(whisper400_six_wide_runs_kernel, whisper400_six_wide_kernel, kSixMaxSlots, LensSix64), kSixWideWaves, six_per_cu, 1},
        MS_FAMILY(whisper400_six_wide_runs_kernel, whisper400_six_wide_kernel, kSixMaxSlots, LensSix40), kSixWideWaves, six_per_cu, 1},
        MS_FAMILY(whisper400_six_wide_runs_kernel, whisper400_six_wide_kernel, kSixWideSlots, LensSix128), kSixWideWaves, 1, 2},       // one twelve-wave workgroup per CU
        MS_FAMILY(whisper400_wave_runs_kernel, whisper400_wave_kernel, 8, LensI80), kWaveWaves, wave_per_cu, 0},
        MS_FAMILY(whisper400_wave_runs_kernel, whisper400_wave_kernel, 8, LensRuntime), kWaveWaves, wave_per_cu, 0},
        MS_FAMILY(whisper400_wave_runs_kernel, whisper400_wave_kernel, 12, LensI128), kWaveWaves, wave_per_cu, 0},
        MS_FAMILY(whisper400_wave_runs_kernel, whisper400_wave_kernel, 12, LensRuntime), kWaveWaves, wave_per_cu, 0}};
#undef MS_FAMILY
    return table[static_cast<int>(k)];
}

// One launch of a member of family f on desc.  io_runs: the 16-bit kernel that takes the run-per-wave member's place (io_kernels allowed it
// the LDS)
int launch_fast(melspec_ctx *c, const BatchDesc &desc, const FixSink &sink, hipStream_t stream, FastFamily &f, FastKernel io_runs = nullptr) {
    if (!f.runs) return fail(MELSPEC_ERR_INTERNAL, "launch_fast: no f32 kernel on this route");
    if (!io_runs)
        if (int rc = allow_big_lds_once(f.done, "hipFuncSetAttribute(whisper400 f32 kernels)", f.runs, f.layout)) return rc;
    const FastTables &ft = f.bank == 0 ? c->ft : f.bank == 1 ? c->ft6 : c->ft6w;
    const DevBuf &blob = f.bank == 0 ? c->d_blob : f.bank == 1 ? c->d_blob6 : c->d_blob6w;
    const size_t lds = f.bank == 0 ? c->fast_lds : f.bank == 1 ? c->lds6 : c->lds6w;
    const uint64_t blocks = (desc.n_units + f.waves - 1) / f.waves;
    const dim3 grid(grid_for_xcd(blocks, c->dev.cus, f.per_cu)), block(f.waves * 64);
    FastParams fp{};
    fp.b = desc;
    fp.d_blob = static_cast<const float *>(blob.p);
    fp.blob_len = static_cast<int>(ft.blob.size());
    fp.hop = c->hop_size;
    fp.n_mels = c->n_mels;
    fp.slice_floats = WaveLayout::slice_floats();
    fp.slots = ft.slots;
    fp.fix = sink_armed(c, sink, desc, grid.x);
    fp.fix.vote_groups = std::min<unsigned>(grid.x, static_cast<unsigned>(c->dev.cus));        // workgroups that are certainly resident when the launch starts
    const bool layout = is_layout(desc);
    hipLaunchKernelGGL(io_runs ? io_runs : layout ? f.layout : f.runs, grid, block, lds, stream, fp);
    HIP_TRY(hipGetLastError());
#ifdef MELSPEC_LAB_STAMPS
    // tools/tail_probe.py: the 200th plain sixteen-wave launch's per-wave end stamps and per-workgroup start stamps, as one line per workgroup
    static int stamp_calls = 0;
    if (f.waves == kSixWaves && !io_runs && !layout && fp.fix.list && lab_int("MELSPEC_LAB_STAMPS", 0, 0, 1) && ++stamp_calls == 200) {
        HIP_TRY(hipStreamSynchronize(stream));
        const size_t n = static_cast<size_t>(grid.x) * kSixWaves + grid.x;
        std::vector<uint64_t> st(n);
        HIP_TRY(hipMemcpy(st.data(), fp.fix.list + desc.n_units + 4096, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
        uint64_t t0 = ~0ull;
        for (unsigned g = 0; g < grid.x; ++g) t0 = std::min(t0, st[static_cast<size_t>(grid.x) * kSixWaves + g]);
        for (unsigned g = 0; g < grid.x; ++g) {
            std::fprintf(stderr, "STAMP wg %u start %llu ends", g, static_cast<unsigned long long>(st[static_cast<size_t>(grid.x) * kSixWaves + g] - t0));
            for (int w = 0; w < kSixWaves; ++w) std::fprintf(stderr, " %llu", static_cast<unsigned long long>(st[static_cast<size_t>(g) * kSixWaves + w] - t0));
            std::fprintf(stderr, "\n");
        }
    }
#endif
    return MELSPEC_OK;
}

// the f64 launch of a route: the whole batch in MELSPEC_PRECISION_F64, or AUTO's gated one
int launch_f64(melspec_ctx *c, const BatchDesc &desc, const FixSink &stat, hipStream_t stream, const Route &r, const IoKernels *iok, const unsigned *gate = nullptr,
               unsigned gate_value = 0) {
    if (!is_six64(r.f64)) return launch_precise(c, desc, stat, stream, r.f64, gate, gate_value);
    Six64Kernel k = nullptr;
    if (iok) k = r.f64 == F64Kernel::kSix64x15 ? iok->f64_128 : iok->f64_80;
    else if (int rc = six64_kernel(r.f64, k)) return rc;
    return launch_six64(c, desc, stat, stream, k, gate, gate_value);
}

BatchKind batch_kind(const BatchDesc &desc, int io) {
    if (io) return BatchKind::kIo;
    if (is_layout(desc)) return desc.d_unit_ext ? BatchKind::kLayoutExt : BatchKind::kLayout;
    return desc.d_unit_prefix ? BatchKind::kRagged : BatchKind::kUniform;
}

int launch_ctx(melspec_ctx *c, const BatchDesc &desc_in, hipStream_t stream, int io) {
    if (desc_in.n_units == 0) return MELSPEC_OK;
    BatchDesc desc = desc_in;
    const IoKernels *iok = nullptr;
    if (io) {
        // the entry points ask ctx_supports_io before they plan: plain batches of the six-frame contexts, planned on the host
        if (!ctx_supports_io(c) || is_layout(desc) || desc.frames_per_unit != kSixFrames || desc.d_n_units != nullptr || desc.d_unit_ext != nullptr)
            return fail(MELSPEC_ERR_INTERNAL, "launch_ctx: a 16-bit batch off the six-frame kernels");
        if (int rc = io_kernels(io, iok)) return rc;
    }
    if (!c->fast) {
        if (desc.sync_rounds < 0) desc.sync_rounds = 1;
        return c->fast512 && desc.frames_per_unit == kFbFPW ? launch_whisper512(c, desc, stream)
                                                            : launch_generic(c->gt, desc, c->hop_size, 0, 1, 1, 0.0, 0.0, c->dev.cus, stream);
    }
    const CtxShape shape = ctx_shape(c);
    const BatchKind kind = batch_kind(desc, io);
    Route r = route400(shape, kind);
    // a batch of the layout entry that came out frame-major and without padding: planned like a layout, stored like a plain batch
    if (kind == BatchKind::kUniform && r.frames_per_unit != desc.frames_per_unit) r = route400(shape, BatchKind::kUnpadded);
    if (r.frames_per_unit != desc.frames_per_unit) return fail(MELSPEC_ERR_INTERNAL, "launch_ctx: the batch was planned for another kernel's unit size");
    if (desc.sync_rounds < 0) desc.sync_rounds = r.sync_rounds;
    if (r.f32 == F32Kernel::kNone) return launch_f64(c, desc, FixSink{}, stream, r, iok);          // MELSPEC_PRECISION_F64
    FixSink sink{};
    if (c->precision == MELSPEC_PRECISION_AUTO)
        if (int rc = auto_sink(c, desc, stream, r.gated, sink)) return rc;
    hipEvent_t pe0 = nullptr, pe1 = nullptr;
    if (c->first_kernel_events) {
        HIP_TRY(hipEventCreate(&pe0)); HIP_TRY(hipEventCreate(&pe1));
        c->first_kernel_events->push_back(pe0); c->first_kernel_events->push_back(pe1);
        HIP_TRY(hipEventRecord(pe0, stream));
    }
    const int rc = launch_fast(c, desc, sink, stream, fast_family(r.f32), !iok ? nullptr : r.f32 == F32Kernel::kSix12x15 ? iok->runs128 : iok->runs80);
    if (pe1) HIP_TRY(hipEventRecord(pe1, stream));
    if (rc || !r.gated) return rc;
    // AUTO's second launch: returns at its first instruction unless the launch above voted "heavy" (its number is c->fix.seq)
    const unsigned gate_value = (c->fix.seq & 0xffffffu) << 2 | kVoteDecided | kVoteHeavy;
    FixSink stat{};
    stat.count = sink.count; stat.acc = sink.acc; stat.host = sink.host;
    BatchDesc d64 = desc_in;
    if (r.replan) d64 = plan_uniform(desc.pcm, desc.out, desc.clip_stride, desc.frames_per_clip, desc.n_clips, c->n_mels, r.replan, desc.out_width, desc.mel_major != 0).desc;
    if (d64.sync_rounds < 0) d64.sync_rounds = r.sync_rounds64;
    return launch_f64(c, d64, stat, stream, r, iok, sink.decision, gate_value);
}

int launch_stft(melspec_ctx *c, const BatchDesc &desc, int bins, int dtype, hipStream_t s) {
    if (desc.n_units == 0) return MELSPEC_OK;
    const int words = bins * 2 * (dtype == MELSPEC_STFT_F64 ? 2 : 1);
    if (c->fast) {
        static std::atomic<uint64_t> attr_done{0};
        if (int rc = allow_big_lds_once(attr_done, "hipFuncSetAttribute(whisper400_stft_kernel)", &whisper400_stft_kernel<float>, &whisper400_stft_kernel<double>)) return rc;
        StftParams p{};
        p.b = desc;
        p.d_blob = static_cast<const uint32_t *>(c->d_blob64s.p);
        p.blob_words = PreciseBlob::kCount * 2;                    // the f64 tables only, not the mel section behind them
        p.hop = c->hop_size; p.bins = bins; p.words_per_frame = words;
        const size_t lds = static_cast<size_t>(p.blob_words) * 4 + static_cast<size_t>(kPreciseWaves) * PreciseLayout::slice_doubles() * sizeof(double);
        const uint64_t blocks = (desc.n_units + kPreciseWaves - 1) / kPreciseWaves;
        const unsigned grid = grid_for_xcd(blocks, c->dev.cus, 1);
        if (dtype == MELSPEC_STFT_F64) hipLaunchKernelGGL(whisper400_stft_kernel<double>, dim3(grid), dim3(kPreciseWaves * 64), lds, s, p);
        else hipLaunchKernelGGL(whisper400_stft_kernel<float>, dim3(grid), dim3(kPreciseWaves * 64), lds, s, p);
        HIP_TRY(hipGetLastError());
        return MELSPEC_OK;
    }
    return launch_generic_stft(c, desc, bins, dtype, s);
}

}  // namespace host
}  // namespace melspec
