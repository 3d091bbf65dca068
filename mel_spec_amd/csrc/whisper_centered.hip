// whisper_centered.hip -- the centred Whisper features (melspec_whisper_*, include/melspec_hip.h has the semantics): the f64 raw kernels
// and the small kernels of whisper_centered_kernels.hpp, their launches and the C ABI.  Default scheduling strategy; the f32 raw kernel is
// emitted by whisper_centered_runs.hip with melspec_runs.hip's.  The kernels with int16 PCM in / f16, bf16 out (melspec_whisper_*_io) are
// emitted by whisper_centered_io.hip / whisper_centered_io_runs.hip and launched from here: one wc_run for all six combinations.
//
// One call is, on its stream:  the tables' upload (the interior's plan through plan_ragged, everything else in one slot of the feature's
// own ring) -> wc_prepare_kernel (maximum words, edge samples) -> the raw kernel on the interior -> the f64 raw kernel on the edge frames
// -> wc_finalize_kernel (normalised calls) or wc_fill_kernel + wc_clip_max_kernel (split calls).
// With the clip table in device memory (the _desc calls, wc_run_desc):  wc_plan_desc_kernel (whisper_desc_kernels.hpp) -> wc_prepare_desc_kernel
// -> plan_ragged_device_kernel + the raw kernel on the interior -> the f64 raw kernel on the edge frames -> the same last passes; nothing is
// uploaded and the launches are sized for the most a table of n_clips clips can ask for.
#include "host_common.hpp"
#include "whisper_centered_io_kernels.hpp"
#include "whisper_desc_kernels.hpp"

namespace melspec {
extern template __global__ void whisper400_six_runs_raw_kernel<kSixMaxSlots, LensSix80>(const WcRawParams);      // whisper_centered_runs.hip
template __global__ void whisper400_six64_raw_kernel<kSixMaxSlots, LensSix80>(const WcRaw64Params);
template __global__ void whisper400_six64_raw_kernel<kSixWideSlots, LensSix128>(const WcRaw64Params);
template __global__ void wc_prepare_kernel<float>(const float *, const host::WcEdge *, uint32_t, float *, int *, uint32_t);
template __global__ void wc_fill_kernel<float>(const host::WcRecord *, float *, int);
template __global__ void wc_finalize_kernel<float>(const host::WcRecord *, const float *, const int *, float *, int, int);
// int16 PCM in / f16, bf16 out: whisper_centered_io_runs.hip, whisper_centered_io.hip
#define MS_IO_EXTERN(In, Out) MS_WC_IO_RUNS(extern template __global__ void, In, Out) MS_WC_IO_64(extern template __global__ void, In, Out)
MS_IO_COMBOS(MS_IO_EXTERN)
#undef MS_IO_EXTERN
MS_WC_IO_SMALL(extern template __global__ void)
// the clip table in device memory (the _desc calls): the gather that reads its count from the plan
template __global__ void wc_prepare_desc_kernel<float>(const float *, const host::WcEdge *, const uint64_t *, uint32_t, float *, int *, uint32_t);
template __global__ void wc_prepare_desc_kernel<io_s16>(const io_s16 *, const host::WcEdge *, const uint64_t *, uint32_t, float *, int *, uint32_t);

__global__ __launch_bounds__(256) void wc_clip_max_kernel(int *slots, uint32_t n) {
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (i < n) reinterpret_cast<float *>(slots)[i] = six_float(slots[i]) - 16.0f;
}

}  // namespace melspec

namespace {

bool wc_supported(const melspec_ctx *c) { return c && ctx_supports_io(c) && c->fft_size == 400 && c->hop_size == 160; }
// the f32 run kernel serves the interior: F32 mode on the 80-mel bank
bool wc_f32(const melspec_ctx *c) { return c->precision == MELSPEC_PRECISION_F32 && c->six && c->six_static == 1; }

int wc_unsupported(const melspec_ctx *c) {
    g_last_error = "the centred Whisper features are computed by the contexts of melspec_create(.., 400, 160, 16000.0, 80 | 128) only; this context is n_fft = " +
                   std::to_string(c->fft_size) + ", hop = " + std::to_string(c->hop_size) + ", n_mels = " + std::to_string(c->n_mels);
    return MELSPEC_ERR_UNSUPPORTED;
}

// ---- the raw kernels of a (sample, row) combination; io = pcm_dtype | out_dtype << 4 (io_dtypes), 0: the f32 kernels -----------------------
typedef void (*WcRaw32)(const WcRawParams);
typedef void (*WcRaw64)(const WcRaw64Params);
struct WcRawKernels {
    WcRaw32 runs80;
    WcRaw64 f64_80, f64_128;
};
template <class In, class Out>
WcRawKernels wc_raw_io_of() {
    return WcRawKernels{&whisper400_six_runs_raw_io_kernel<kSixMaxSlots, LensSix80, In, Out>, &whisper400_six64_raw_io_kernel<kSixMaxSlots, LensSix80, In, Out>,
                        &whisper400_six64_raw_io_kernel<kSixWideSlots, LensSix128, In, Out>};
}
// the kernels are allowed the whole LDS once per device and combination
int wc_raw_kernels(int io, const WcRawKernels *&k) {
    static const WcRawKernels table[2][3] = {
        {WcRawKernels{&whisper400_six_runs_raw_kernel<kSixMaxSlots, LensSix80>, &whisper400_six64_raw_kernel<kSixMaxSlots, LensSix80>,
                      &whisper400_six64_raw_kernel<kSixWideSlots, LensSix128>},
         wc_raw_io_of<float, io_f16>(), wc_raw_io_of<float, io_bf16>()},
        {wc_raw_io_of<io_s16, float>(), wc_raw_io_of<io_s16, io_f16>(), wc_raw_io_of<io_s16, io_bf16>()}};
    static std::atomic<uint64_t> attr_done[2][3];
    const int pcm = io & 15, out = io >> 4;
    if (pcm < 0 || pcm > 1 || out < 0 || out > 2) return fail(MELSPEC_ERR_INTERNAL, "wc_raw_kernels: no such combination");
    k = &table[pcm][out];
    return allow_big_lds_once(attr_done[pcm][out], "hipFuncSetAttribute(whisper400 raw kernels)", k->runs80, k->f64_80, k->f64_128);
}

// the f64 raw kernel on a six-frame plan (launch_six64's shape)
int wc_launch64(melspec_ctx *c, const BatchDesc &desc, int *slots, const uint32_t *slot_map, hipStream_t s, int io) {
    if (desc.n_units == 0) return MELSPEC_OK;
    const WcRawKernels *k = nullptr;
    if (int rc = wc_raw_kernels(io, k)) return rc;
    const uint64_t blocks = (desc.n_units + kSix64Waves - 1) / kSix64Waves;
    const unsigned grid = grid_for_xcd(blocks, c->dev.cus, 1);
    WcRaw64Params q{};
    q.f.b = desc;
    q.f.d_blob = static_cast<const uint32_t *>(c->d_blob64x.p);
    q.f.blob_words = static_cast<int>(c->t64.blob.size());
    q.f.mel_off_words = c->t64.mel_off_words;
    q.f.hop = c->hop_size;
    q.f.n_mels = c->n_mels;
    q.f.slots = c->ft6.slots;
    q.slots = slots; q.slot_map = slot_map;
    hipLaunchKernelGGL(c->six64_wide ? k->f64_128 : k->f64_80, dim3(grid), dim3(kSix64Waves * 64), c->lds64x, s, q);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// the f32 raw kernel (launch_fast's shape for the sixteen-wave family; no guard, no vote)
int wc_launch32(melspec_ctx *c, const BatchDesc &desc, int *slots, hipStream_t s, int io) {
    if (desc.n_units == 0) return MELSPEC_OK;
    const WcRawKernels *k = nullptr;
    if (int rc = wc_raw_kernels(io, k)) return rc;
    const uint64_t blocks = (desc.n_units + kSixWaves - 1) / kSixWaves;
    const unsigned grid = grid_for_xcd(blocks, c->dev.cus, 1);
    WcRawParams q{};
    q.f.b = desc;
    q.f.d_blob = static_cast<const float *>(c->d_blob6.p);
    q.f.blob_len = static_cast<int>(c->ft6.blob.size());
    q.f.hop = c->hop_size;
    q.f.n_mels = c->n_mels;
    q.f.slice_floats = WaveLayout::slice_floats();
    q.f.slots = c->ft6.slots;
    q.slots = slots; q.slot_map = nullptr;
    hipLaunchKernelGGL(k->runs80, dim3(grid), dim3(kSixWaves * 64), c->lds6, s, q);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// ---- the small kernels by the call's types -------------------------------------------------------------------------------------------------
void wc_prepare(const void *d_pcm, int pcm_dtype, const WcEdge *d_edges, uint32_t n_edges, float *d_edge_pcm, int *d_slots, uint32_t n_clips, hipStream_t s) {
    const dim3 grid(n_edges + (n_clips + 255) / 256);
    if (pcm_dtype == MELSPEC_PCM_S16)
        hipLaunchKernelGGL(wc_prepare_kernel<io_s16>, grid, dim3(256), 0, s, static_cast<const io_s16 *>(d_pcm), d_edges, n_edges, d_edge_pcm, d_slots, n_clips);
    else
        hipLaunchKernelGGL(wc_prepare_kernel<float>, grid, dim3(256), 0, s, static_cast<const float *>(d_pcm), d_edges, n_edges, d_edge_pcm, d_slots, n_clips);
}
void wc_fill(const WcRecord *d_rec, void *d_rows, int out_dtype, int nm, dim3 grid, hipStream_t s) {
    if (out_dtype == MELSPEC_OUT_F16) hipLaunchKernelGGL(wc_fill_kernel<io_f16>, grid, dim3(256), 0, s, d_rec, static_cast<io_f16 *>(d_rows), nm);
    else if (out_dtype == MELSPEC_OUT_BF16) hipLaunchKernelGGL(wc_fill_kernel<io_bf16>, grid, dim3(256), 0, s, d_rec, static_cast<io_bf16 *>(d_rows), nm);
    else hipLaunchKernelGGL(wc_fill_kernel<float>, grid, dim3(256), 0, s, d_rec, static_cast<float *>(d_rows), nm);
}
void wc_finalize(const WcRecord *d_rec, const float *d_rows, const int *d_slots, void *d_out, int out_dtype, int nm, int mel_major, dim3 grid, hipStream_t s) {
    const size_t lds = mel_major ? static_cast<size_t>(nm) * (kWcTile + 1) * sizeof(float) : 0;
    if (out_dtype == MELSPEC_OUT_F16)
        hipLaunchKernelGGL(wc_finalize_kernel<io_f16>, grid, dim3(256), lds, s, d_rec, d_rows, d_slots, static_cast<io_f16 *>(d_out), nm, mel_major);
    else if (out_dtype == MELSPEC_OUT_BF16)
        hipLaunchKernelGGL(wc_finalize_kernel<io_bf16>, grid, dim3(256), lds, s, d_rec, d_rows, d_slots, static_cast<io_bf16 *>(d_out), nm, mel_major);
    else
        hipLaunchKernelGGL(wc_finalize_kernel<float>, grid, dim3(256), lds, s, d_rec, d_rows, d_slots, static_cast<float *>(d_out), nm, mel_major);
}

// The batch.  ragged: h_offsets / h_lengths [n_clips]; otherwise clip i = d_pcm + i * clip_stride, clip_len samples.  split: d_dst = the
// caller's raw rows (dst_offsets: where each clip's start, nullptr: packed) and d_clip_max its maxima; otherwise d_dst = the normalised output.
// pcm_dtype / out_dtype: the element types of d_pcm and d_dst (MELSPEC_PCM_* / MELSPEC_OUT_*; every offset, stride and length counts
// elements of them).  (F32, F32) launches exactly what the f32 calls always did.  The raw rows of a normalised call are the scratch's, f32
// whatever out_dtype is, and so are the gathered edge samples: the interior launch is the (pcm_dtype, rows) kernel, the edge launch the
// (F32, rows) one, and out_dtype reaches the split calls' row stores and the fill / finalise passes.
int wc_run(melspec_ctx *c, const void *d_pcm, int pcm_dtype, bool ragged, const uint64_t *h_offsets, const uint64_t *h_lengths, uint64_t clip_stride, uint64_t clip_len,
           uint32_t n_clips, uint64_t pad_to, void *d_dst, int out_dtype, const uint64_t *dst_offsets, bool split, float *d_clip_max, int mel_major, void *stream) {
    uint64_t total = 0;
    if (c && wc_supported(c) && wc_pad_ok(pad_to) && (!ragged || (h_offsets && h_lengths)))
        for (uint32_t i = 0; i < n_clips; ++i) total += wc_num_frames(ragged ? h_lengths[i] : clip_len, pad_to);
    const WcArgs a = wc_args_io(c != nullptr, c && wc_supported(c), pcm_dtype, out_dtype, pad_to, ragged, n_clips, h_offsets, h_lengths, clip_stride, clip_len, total, d_pcm,
                                d_dst, split, d_clip_max);
    if (a.verdict == kWcFail) return a.msg ? fail(a.status, a.msg) : wc_unsupported(c);
    if (a.verdict == kWcDone) return MELSPEC_OK;
    HIP_TRY(hipSetDevice(c->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (a.verdict == kWcSlots) {          // no clip has a frame: the maxima alone
        wc_prepare(nullptr, MELSPEC_PCM_F32, nullptr, 0u, nullptr, reinterpret_cast<int *>(d_clip_max), n_clips, s);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(wc_clip_max_kernel, dim3((n_clips + 255) / 256), dim3(256), 0, s, reinterpret_cast<int *>(d_clip_max), n_clips);
        HIP_TRY(hipGetLastError());
        return MELSPEC_OK;
    }
    const int nm = c->n_mels;
    // the split calls' rows go where the caller says; the normalised calls' raw rows are packed in the scratch
    const WcBatch b = wc_plan(ragged ? h_offsets : nullptr, ragged ? h_lengths : &clip_len, clip_stride, n_clips, pad_to, nm, split ? dst_offsets : nullptr, split ? nullptr : dst_offsets);
    if (b.edges.size() > 0xffffffffull) return fail(MELSPEC_ERR_INVALID_ARG, "too many clips for one call");
    const uint32_t n_edges = static_cast<uint32_t>(b.edges.size());
    int rc;
    void *d_rows = d_dst;
    const int rows_dtype = split ? out_dtype : MELSPEC_OUT_F32;
    const int io_interior = pcm_dtype | rows_dtype << 4, io_edge = MELSPEC_PCM_F32 | rows_dtype << 4;
    int *d_slots = reinterpret_cast<int *>(d_clip_max);
    if (!split) {
        if ((rc = c->wc.rows.ensure(b.rows_floats * sizeof(float), s))) return rc;
        if ((rc = c->wc.slots.ensure(static_cast<size_t>(n_clips) * sizeof(int), s))) return rc;
        d_rows = c->wc.rows.p();
        d_slots = static_cast<int *>(c->wc.slots.p());
    }
    if ((rc = c->wc.edge_pcm.ensure((static_cast<size_t>(n_edges) + 1) * kWcFft * sizeof(float), s))) return rc;
    float *d_edge_pcm = static_cast<float *>(c->wc.edge_pcm.p());

    // one slot: the clip records, the edge frames, and the edge launch's batch -- every edge frame a "clip" of one frame whose samples are
    // edge_pcm + 400 e and whose row is the frame's (d_off, d_frames, d_out_off, d_unit_prefix [n + 1], then d_unit_block and the words'
    // map as 32-bit entries)
    const size_t rec_bytes = round16(static_cast<size_t>(n_clips) * sizeof(WcRecord)), edge_bytes = round16(static_cast<size_t>(n_edges) * sizeof(WcEdge));
    const size_t e64 = static_cast<size_t>(n_edges) * 4 + 1 + 4;         // (+ 4: locate's look-ahead past the last clip stays inside the slot)
    const size_t eblk = (static_cast<size_t>(n_edges) + kUnitBlock - 1) / kUnitBlock + 1;
    const size_t plan_bytes = round16(e64 * sizeof(uint64_t) + (eblk + n_edges) * sizeof(uint32_t));
    const size_t bytes = rec_bytes + edge_bytes + plan_bytes;
    RaggedSlot *sl = nullptr;
    if ((rc = table_slot_take(c->wc.ring, bytes, sl))) return rc;
    {
        char *h = static_cast<char *>(sl->host);
        std::memset(h, 0, bytes);
        if (n_clips) std::memcpy(h, b.records.data(), static_cast<size_t>(n_clips) * sizeof(WcRecord));
        if (n_edges) std::memcpy(h + rec_bytes, b.edges.data(), static_cast<size_t>(n_edges) * sizeof(WcEdge));
        uint64_t *off = reinterpret_cast<uint64_t *>(h + rec_bytes + edge_bytes), *fr = off + n_edges, *oo = fr + n_edges, *pre = oo + n_edges;
        uint32_t *blk = reinterpret_cast<uint32_t *>(off + e64), *map = blk + eblk;
        for (uint32_t e = 0; e < n_edges; ++e) {
            off[e] = static_cast<uint64_t>(e) * kWcFft; fr[e] = 1; oo[e] = b.edges[e].row_off; pre[e] = e;
            map[e] = static_cast<uint32_t>(b.edges[e].clip);
        }
        pre[n_edges] = n_edges;
        for (size_t k = 0; k + 1 < eblk; ++k) blk[k] = static_cast<uint32_t>(k * kUnitBlock);
    }
    if ((rc = table_slot_upload(*sl, bytes, s))) { plan_ragged_done(sl, s); return rc; }
    const char *dt = static_cast<const char *>(sl->dev.p);
    const WcRecord *d_rec = reinterpret_cast<const WcRecord *>(dt);
    const WcEdge *d_edges = reinterpret_cast<const WcEdge *>(dt + rec_bytes);
    const uint64_t *d_e64 = reinterpret_cast<const uint64_t *>(dt + rec_bytes + edge_bytes);
    const uint32_t *d_eblk = reinterpret_cast<const uint32_t *>(d_e64 + e64), *d_map = d_eblk + eblk;

    RaggedSlot *in_slot = nullptr;
    auto done = [&](int code) { plan_ragged_done(sl, s); plan_ragged_done(in_slot, s); return code; };

    wc_prepare(d_pcm, pcm_dtype, d_edges, n_edges, d_edge_pcm, d_slots, n_clips, s);
    if (hipGetLastError() != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "wc_prepare_kernel launch failed"));

    // the interior: a plain ragged batch of un-centred frames for the existing planner
    if (b.interior_frames) {
        BatchPlan pl;
        if ((rc = plan_ragged(c->ragged, s, static_cast<const float *>(d_pcm), static_cast<float *>(d_rows), b.in_off.data(), b.in_frames, b.in_out_off.data(), n_clips, nm, kSixFrames, pl, in_slot))) return done(rc);
        if ((rc = wc_f32(c) ? wc_launch32(c, pl.desc, d_slots, s, io_interior) : wc_launch64(c, pl.desc, d_slots, nullptr, s, io_interior))) return done(rc);
    }
    // the edge frames, in f64 whatever the mode
    if (n_edges) {
        BatchDesc d{};
        d.pcm = d_edge_pcm; d.out = static_cast<float *>(d_rows); d.n_clips = n_edges; d.n_units = n_edges; d.frames_per_unit = kSixFrames;
        d.d_off = d_e64; d.d_frames = d_e64 + n_edges; d.d_out_off = d_e64 + 2 * static_cast<size_t>(n_edges); d.d_unit_prefix = d_e64 + 3 * static_cast<size_t>(n_edges);
        d.d_unit_block = d_eblk;
        d.stat_frames = n_edges;
        if ((rc = wc_launch64(c, d, d_slots, d_map, s, io_edge))) return done(rc);
    }
    const unsigned tiles = static_cast<unsigned>(std::min<uint64_t>((b.max_T + kWcTile - 1) / kWcTile, 65535));
    if (split) {
        if (b.silent_frames) {
            wc_fill(d_rec, d_rows, out_dtype, nm, dim3(n_clips, tiles), s);
            if (hipGetLastError() != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "wc_fill_kernel launch failed"));
        }
        hipLaunchKernelGGL(wc_clip_max_kernel, dim3((n_clips + 255) / 256), dim3(256), 0, s, d_slots, n_clips);
        if (hipGetLastError() != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "wc_clip_max_kernel launch failed"));
    } else {
        wc_finalize(d_rec, static_cast<const float *>(d_rows), d_slots, d_dst, out_dtype, nm, mel_major ? 1 : 0, dim3(n_clips, tiles), s);
        if (hipGetLastError() != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "wc_finalize_kernel launch failed"));
    }
    return done(MELSPEC_OK);
}

// The same batch with its tables in device memory (the _desc calls): d_offsets / d_lengths [n_clips] and the optional dst_offsets are read
// by wc_plan_desc_kernel on the stream; the host reads none of them and waits for nothing.  pad_to >= 400 fixes T, so the outputs' sizes,
// the packed offsets and every scratch size are the host's; the classes of the frames are not, so the launches are sized for the most
// there can be -- T - 2 interior frames and five edge frames per clip, the true counts at BatchDesc::d_n_units -- and the fill pass and
// the interior launch run whatever the table holds.  Kernel choice, maximum words and the f64 edge launch: wc_run's.
int wc_run_desc(melspec_ctx *c, bool io, const void *d_pcm, int pcm_dtype, const uint64_t *d_offsets, const uint64_t *d_lengths, uint32_t n_clips, uint64_t pad_to,
                void *d_dst, int out_dtype, const uint64_t *d_dst_offsets, bool split, float *d_clip_max, int mel_major, void *stream) {
    const WcArgs a = wc_args_desc_io(c != nullptr, c && wc_supported(c), io, pcm_dtype, out_dtype, pad_to, n_clips, d_offsets, d_lengths, d_pcm, d_dst, split, d_clip_max);
    if (a.verdict == kWcFail) return a.msg ? fail(a.status, a.msg) : wc_unsupported(c);
    if (a.verdict == kWcDone) return MELSPEC_OK;
    HIP_TRY(hipSetDevice(c->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const int nm = c->n_mels;
    const uint64_t T = pad_to / kWcHop;
    const uint32_t cap = static_cast<uint32_t>(wc_desc_cap(n_clips));
    int rc;
    void *d_rows = d_dst;
    const int rows_dtype = split ? out_dtype : MELSPEC_OUT_F32;
    const int io_interior = pcm_dtype | rows_dtype << 4, io_edge = MELSPEC_PCM_F32 | rows_dtype << 4;
    int *d_slots = reinterpret_cast<int *>(d_clip_max);
    if (!split) {
        if ((rc = c->wc.rows.ensure(static_cast<size_t>(n_clips) * T * nm * sizeof(float), s))) return rc;
        if ((rc = c->wc.slots.ensure(static_cast<size_t>(n_clips) * sizeof(int), s))) return rc;
        d_rows = c->wc.rows.p();
        d_slots = static_cast<int *>(c->wc.slots.p());
    }
    if ((rc = c->wc.edge_pcm.ensure((static_cast<size_t>(cap) + 1) * kWcFft * sizeof(float), s))) return rc;
    float *d_edge_pcm = static_cast<float *>(c->wc.edge_pcm.p());

    // the plan: DevicePlan's rule -- in stream order, a call on another stream first waits for the stream that used the buffer last
    DevicePlan &dp = c->wc.dtab;
    const size_t bytes = wc_desc_bytes(n_clips);
    if (dp.used && dp.last != s) HIP_TRY(hipStreamSynchronize(dp.last));
    if (bytes > dp.buf.cap && dp.used) HIP_TRY(hipStreamSynchronize(dp.last));
    if ((rc = dp.buf.ensure(bytes))) return rc;
    dp.used = true; dp.last = s;
    WcPlanDescParams q{};
    q.in.off = d_offsets; q.in.len = d_lengths;
    q.in.rows_off = split ? d_dst_offsets : nullptr; q.in.out_off = split ? nullptr : d_dst_offsets;
    q.in.n_clips = n_clips; q.in.n_mels = static_cast<uint32_t>(nm); q.in.pad_to = pad_to;
    q.plan = dp.buf.p;
    hipLaunchKernelGGL(wc_plan_desc_kernel, dim3(1), dim3(kWcDescThreads), 0, s, q);
    HIP_TRY(hipGetLastError());
    const WcDescTables t = wc_desc_tables(dp.buf.p, n_clips);

    {
        const dim3 grid(static_cast<unsigned>(std::min<uint64_t>(static_cast<uint64_t>(cap) + (n_clips + 255) / 256, 0x7fffffffull)));          // grid-stride past the limit
        if (pcm_dtype == MELSPEC_PCM_S16)
            hipLaunchKernelGGL(wc_prepare_desc_kernel<io_s16>, grid, dim3(256), 0, s, static_cast<const io_s16 *>(d_pcm), t.edges, t.n_edges, cap, d_edge_pcm, d_slots, n_clips);
        else
            hipLaunchKernelGGL(wc_prepare_desc_kernel<float>, grid, dim3(256), 0, s, static_cast<const float *>(d_pcm), t.edges, t.n_edges, cap, d_edge_pcm, d_slots, n_clips);
        HIP_TRY(hipGetLastError());
    }
    // the interior: the plan's (offset + 120, length, rows two rows in) through the planner of melspec_compute_ragged_device_desc, into a
    // buffer of this feature's own
    const uint64_t bound = wc_desc_interior_bound(n_clips, pad_to);
    if (bound) {
        BatchPlan pl;
        if ((rc = plan_ragged_device(c->wc.dplan, s, static_cast<const float *>(d_pcm), static_cast<float *>(d_rows), t.in_off, t.in_len, t.in_out_off, n_clips, kWcFft, kWcHop,
                                     static_cast<uint32_t>(nm), kSixFrames, bound, pl)))
            return rc;
        if ((rc = wc_f32(c) ? wc_launch32(c, pl.desc, d_slots, s, io_interior) : wc_launch64(c, pl.desc, d_slots, nullptr, s, io_interior))) return rc;
    }
    // the edge frames, in f64 whatever the mode: five slots per clip, the true count on the device
    {
        BatchDesc d{};
        d.pcm = d_edge_pcm; d.out = static_cast<float *>(d_rows); d.n_clips = cap; d.n_units = cap; d.frames_per_unit = kSixFrames;
        d.d_off = t.e_off; d.d_frames = t.e_frames; d.d_out_off = t.e_out_off; d.d_unit_prefix = t.e_prefix;
        d.d_unit_block = t.e_blk;
        d.d_n_units = t.n_edges;
        if ((rc = wc_launch64(c, d, d_slots, t.e_map, s, io_edge))) return rc;
    }
    const unsigned tiles = static_cast<unsigned>(std::min<uint64_t>((T + kWcTile - 1) / kWcTile, 65535));
    if (split) {
        wc_fill(t.rec, d_rows, out_dtype, nm, dim3(n_clips, tiles), s);
        if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, "wc_fill_kernel launch failed");
        hipLaunchKernelGGL(wc_clip_max_kernel, dim3((n_clips + 255) / 256), dim3(256), 0, s, d_slots, n_clips);
        if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, "wc_clip_max_kernel launch failed");
    } else {
        wc_finalize(t.rec, static_cast<const float *>(d_rows), d_slots, d_dst, out_dtype, nm, mel_major ? 1 : 0, dim3(n_clips, tiles), s);
        if (hipGetLastError() != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, "wc_finalize_kernel launch failed");
    }
    return MELSPEC_OK;
}

}  // namespace

extern "C" {

int melspec_whisper_supports(const melspec_ctx *c) { return wc_supported(c) ? 1 : 0; }

size_t melspec_whisper_num_frames(const melspec_ctx *c, size_t n_samples, size_t pad_to) {
    if (!wc_supported(c) || !wc_pad_ok(pad_to)) return 0;
    return static_cast<size_t>(wc_num_frames(n_samples, pad_to));
}

const char *melspec_whisper_kernel_name(const melspec_ctx *c) {
    if (!wc_supported(c)) return "";
    if (wc_f32(c)) return "melspec::whisper400_six_runs_raw_kernel<9, LensSix80> (raw rows + clip maximum; edge frames: whisper400_six64_raw_kernel<9, LensSix80>)";
    return c->six64_wide ? "melspec::whisper400_six64_raw_kernel<15, LensSix128> (f64 FFT, raw rows + clip maximum)"
                         : "melspec::whisper400_six64_raw_kernel<9, LensSix80> (f64 FFT, raw rows + clip maximum)";
}

int melspec_whisper_supports_io(const melspec_ctx *c, int pcm_dtype, int out_dtype) {
    return wc_supported(c) && wc_pcm_known(pcm_dtype) && wc_out_known(out_dtype) ? 1 : 0;
}

int melspec_whisper_compute_uniform_device(melspec_ctx *c, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips, uint64_t pad_to,
                                           float *d_out, int mel_major, void *stream) {
    return wc_run(c, d_pcm, MELSPEC_PCM_F32, false, nullptr, nullptr, clip_stride, clip_len, n_clips, pad_to, d_out, MELSPEC_OUT_F32, nullptr, false, nullptr, mel_major, stream);
}
int melspec_whisper_compute_ragged_device(melspec_ctx *c, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                          uint64_t pad_to, float *d_out, const uint64_t *h_out_offsets, int mel_major, void *stream) {
    return wc_run(c, d_pcm, MELSPEC_PCM_F32, true, h_offsets, h_lengths, 0, 0, n_clips, pad_to, d_out, MELSPEC_OUT_F32, h_out_offsets, false, nullptr, mel_major, stream);
}
int melspec_whisper_compute_uniform_device_split(melspec_ctx *c, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips, uint64_t pad_to,
                                                 float *d_rows, float *d_clip_max, void *stream) {
    return wc_run(c, d_pcm, MELSPEC_PCM_F32, false, nullptr, nullptr, clip_stride, clip_len, n_clips, pad_to, d_rows, MELSPEC_OUT_F32, nullptr, true, d_clip_max, 0, stream);
}
int melspec_whisper_compute_ragged_device_split(melspec_ctx *c, const float *d_pcm, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                                uint64_t pad_to, float *d_rows, const uint64_t *h_rows_offsets, float *d_clip_max, void *stream) {
    return wc_run(c, d_pcm, MELSPEC_PCM_F32, true, h_offsets, h_lengths, 0, 0, n_clips, pad_to, d_rows, MELSPEC_OUT_F32, h_rows_offsets, true, d_clip_max, 0, stream);
}

int melspec_whisper_compute_uniform_device_io(melspec_ctx *c, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                              uint64_t pad_to, void *d_out, int out_dtype, int mel_major, void *stream) {
    return wc_run(c, d_pcm, pcm_dtype, false, nullptr, nullptr, clip_stride, clip_len, n_clips, pad_to, d_out, out_dtype, nullptr, false, nullptr, mel_major, stream);
}
int melspec_whisper_compute_ragged_device_io(melspec_ctx *c, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                             uint32_t n_clips, uint64_t pad_to, void *d_out, int out_dtype, const uint64_t *h_out_offsets, int mel_major, void *stream) {
    return wc_run(c, d_pcm, pcm_dtype, true, h_offsets, h_lengths, 0, 0, n_clips, pad_to, d_out, out_dtype, h_out_offsets, false, nullptr, mel_major, stream);
}
int melspec_whisper_compute_uniform_device_split_io(melspec_ctx *c, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                                    uint64_t pad_to, void *d_rows, int out_dtype, float *d_clip_max, void *stream) {
    return wc_run(c, d_pcm, pcm_dtype, false, nullptr, nullptr, clip_stride, clip_len, n_clips, pad_to, d_rows, out_dtype, nullptr, true, d_clip_max, 0, stream);
}
int melspec_whisper_compute_ragged_device_split_io(melspec_ctx *c, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets, const uint64_t *h_lengths,
                                                   uint32_t n_clips, uint64_t pad_to, void *d_rows, int out_dtype, const uint64_t *h_rows_offsets, float *d_clip_max,
                                                   void *stream) {
    return wc_run(c, d_pcm, pcm_dtype, true, h_offsets, h_lengths, 0, 0, n_clips, pad_to, d_rows, out_dtype, h_rows_offsets, true, d_clip_max, 0, stream);
}

// ---- the clip table in device memory ---------------------------------------------------------------------------------------------------------
int melspec_whisper_supports_desc(const melspec_ctx *c) { return wc_supported(c) ? 1 : 0; }

int melspec_whisper_compute_ragged_device_desc(melspec_ctx *c, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths, uint32_t n_clips,
                                               uint64_t pad_to, float *d_out, const uint64_t *d_out_offsets, int mel_major, void *stream) {
    return wc_run_desc(c, false, d_pcm, MELSPEC_PCM_F32, d_offsets, d_lengths, n_clips, pad_to, d_out, MELSPEC_OUT_F32, d_out_offsets, false, nullptr, mel_major, stream);
}
int melspec_whisper_compute_ragged_device_desc_split(melspec_ctx *c, const float *d_pcm, const uint64_t *d_offsets, const uint64_t *d_lengths, uint32_t n_clips,
                                                     uint64_t pad_to, float *d_rows, const uint64_t *d_rows_offsets, float *d_clip_max, void *stream) {
    return wc_run_desc(c, false, d_pcm, MELSPEC_PCM_F32, d_offsets, d_lengths, n_clips, pad_to, d_rows, MELSPEC_OUT_F32, d_rows_offsets, true, d_clip_max, 0, stream);
}
int melspec_whisper_compute_ragged_device_desc_io(melspec_ctx *c, const void *d_pcm, int pcm_dtype, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                                  uint32_t n_clips, uint64_t pad_to, void *d_out, int out_dtype, const uint64_t *d_out_offsets, int mel_major,
                                                  void *stream) {
    return wc_run_desc(c, true, d_pcm, pcm_dtype, d_offsets, d_lengths, n_clips, pad_to, d_out, out_dtype, d_out_offsets, false, nullptr, mel_major, stream);
}
int melspec_whisper_compute_ragged_device_desc_split_io(melspec_ctx *c, const void *d_pcm, int pcm_dtype, const uint64_t *d_offsets, const uint64_t *d_lengths,
                                                        uint32_t n_clips, uint64_t pad_to, void *d_rows, int out_dtype, const uint64_t *d_rows_offsets,
                                                        float *d_clip_max, void *stream) {
    return wc_run_desc(c, true, d_pcm, pcm_dtype, d_offsets, d_lengths, n_clips, pad_to, d_rows, out_dtype, d_rows_offsets, true, d_clip_max, 0, stream);
}

}  // extern "C"

namespace {
// one clip from host memory: the bytes of the call's own types cross the bus
int wc_host(melspec_ctx *c, const void *samples, int pcm_dtype, size_t n_samples, size_t pad_to, void *out, int out_dtype, size_t out_capacity_elems, int mel_major,
            size_t *n_frames) {
    if (n_frames) *n_frames = 0;
    if (!c) return fail(MELSPEC_ERR_INVALID_ARG, "ctx is NULL");
    int io;
    if (int rc = io_dtypes(pcm_dtype, out_dtype, io)) return rc;
    if (!wc_supported(c)) return wc_unsupported(c);
    if (!wc_pad_ok(pad_to)) return fail(MELSPEC_ERR_INVALID_ARG, "pad_to must be 0 or at least 400");
    const uint64_t T = wc_num_frames(n_samples, pad_to);
    const uint64_t n_up = pad_to && n_samples > pad_to ? pad_to : n_samples;        // what the call reads of the clip
    if (T && n_up && !samples) return fail(MELSPEC_ERR_INVALID_ARG, "samples/out is NULL");
    static const float nothing[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int rc = host_one_clip(c->dev.device, c->wc_h2d, c->wc_d2h, c->stream, n_up ? samples : nothing, n_up ? n_up * wc_pcm_bytes(pcm_dtype) : sizeof(nothing), out,
                                 out_capacity_elems, T * static_cast<uint64_t>(c->n_mels), wc_out_bytes(out_dtype), [&](void *d_in, void *d_out) {
                                     return wc_run(c, d_in, pcm_dtype, false, nullptr, nullptr, n_up, n_up, 1, pad_to, d_out, out_dtype, nullptr, false, nullptr, mel_major,
                                                   c->stream);
                                 });
    if (!rc && n_frames) *n_frames = static_cast<size_t>(T);
    return rc;
}
}  // namespace

extern "C" {

int melspec_whisper_compute_host(melspec_ctx *c, const float *samples, size_t n_samples, size_t pad_to, float *out, size_t out_capacity_floats, int mel_major,
                                 size_t *n_frames) {
    return wc_host(c, samples, MELSPEC_PCM_F32, n_samples, pad_to, out, MELSPEC_OUT_F32, out_capacity_floats, mel_major, n_frames);
}
int melspec_whisper_compute_host_io(melspec_ctx *c, const void *samples, int pcm_dtype, size_t n_samples, size_t pad_to, void *out, int out_dtype,
                                    size_t out_capacity_elems, int mel_major, size_t *n_frames) {
    return wc_host(c, samples, pcm_dtype, n_samples, pad_to, out, out_dtype, out_capacity_elems, mel_major, n_frames);
}

}  // extern "C"
