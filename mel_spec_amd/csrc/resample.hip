// resample.hip -- the C ABI of the polyphase resampler (include/melspec_resample.h): 8-96 kHz PCM, int16 or f32, to f32 PCM at the model
// rate, in HBM, on the caller's stream, ready for the frontends' device calls.  resample_plan.hpp: the definition, the tap table, the
// clip table and the tiles (host-testable); resample_kernels.hpp: the kernel.  A translation unit of its own: no existing kernel is
// compiled differently.
#include "host_common.hpp"
#include "../../include/melspec_resample.h"
#include "resample_kernels.hpp"

struct melspec_resampler {
    DeviceInfo dev;
    RsGeom g;
    RsLaunch l;
    hipStream_t stream = nullptr;
    DevBuf d_win, d_start;      // RsTable
    RaggedScratch ring;         // the clip tables' way to the device
    DevBuf h2d, d2h;            // melspec_resample_host's staging
};

namespace {

int rs_status(int rc) {
    if (rc == MELSPEC_ERR_INVALID_ARG) return fail(rc, "rate_in and rate_out must be at least 1");
    if (rc == MELSPEC_ERR_UNSUPPORTED) return fail(rc, "rate_in / gcd or rate_out / gcd is above 4096");
    return rc;
}

template <class S, int MODE>
void rs_launch_one(const melspec_resampler *r, unsigned grid, hipStream_t s, const void *d_pcm, float *d_out, const RsClip *d_tab, uint32_t n_clips, uint64_t n_tiles) {
    const RsKernelGeom kg{r->g.orig, r->g.nw, r->g.width, r->g.taps, r->l.blocks};
    hipLaunchKernelGGL((resample_kernel<S, MODE>), dim3(grid), dim3(kRsThreads), r->l.lds, s, static_cast<const S *>(d_pcm), d_out, d_tab, n_clips, n_tiles, kg,
                       static_cast<const double *>(r->d_win.p), static_cast<const uint32_t *>(r->d_start.p));
}
template <class S>
void rs_launch_mode(const melspec_resampler *r, unsigned grid, hipStream_t s, const void *d_pcm, float *d_out, const RsClip *d_tab, uint32_t n_clips, uint64_t n_tiles) {
    switch (r->l.mode) {
        case kRsLdsAll: rs_launch_one<S, kRsLdsAll>(r, grid, s, d_pcm, d_out, d_tab, n_clips, n_tiles); break;
        case kRsLdsSamples: rs_launch_one<S, kRsLdsSamples>(r, grid, s, d_pcm, d_out, d_tab, n_clips, n_tiles); break;
        case kRsGlobal: rs_launch_one<S, kRsGlobal>(r, grid, s, d_pcm, d_out, d_tab, n_clips, n_tiles); break;
        default: rs_launch_one<S, kRsCopy>(r, grid, s, d_pcm, d_out, d_tab, n_clips, n_tiles); break;
    }
}

// a checked batch (offsets == NULL: uniform) on stream s: the table through a ring slot, one launch
int rs_run(melspec_resampler *r, const void *d_pcm, int pcm_dtype, const uint64_t *offsets, const uint64_t *lengths, const uint64_t *out_offsets,
           uint64_t clip_stride, uint64_t clip_len, uint64_t out_stride, uint32_t n_clips, float *d_out, hipStream_t s) {
    HIP_TRY(hipSetDevice(r->dev.device));
    const size_t bytes = (static_cast<size_t>(n_clips) + 1) * sizeof(RsClip);
    static_assert(sizeof(RsClip) % 16 == 0, "the ring's slots travel in 16-byte words");
    RaggedSlot *sl = nullptr;
    if (int rc = table_slot_take(r->ring, bytes, sl)) return rc;
    const uint64_t n_tiles = rs_plan(r->g, r->l, offsets, lengths, out_offsets, clip_stride, clip_len, out_stride, n_clips, static_cast<RsClip *>(sl->host));
    if (n_tiles == 0) return MELSPEC_OK;
    if (int rc = table_slot_upload(*sl, bytes, s)) return rc;
    const size_t lds = r->l.lds ? r->l.lds : 1;
    const int per_cu = static_cast<int>(std::min<size_t>(8, std::max<size_t>(1, kLdsLimit / lds)));
    const unsigned grid = grid_for(n_tiles, r->dev.cus, per_cu);
    if (pcm_dtype == MELSPEC_PCM_S16) rs_launch_mode<io_s16>(r, grid, s, d_pcm, d_out, static_cast<const RsClip *>(sl->dev.p), n_clips, n_tiles);
    else rs_launch_mode<float>(r, grid, s, d_pcm, d_out, static_cast<const RsClip *>(sl->dev.p), n_clips, n_tiles);
    const hipError_t e = hipGetLastError();
    plan_ragged_done(sl, s);
    if (e != hipSuccess) return fail_hip(e, "resample_kernel launch");
    return MELSPEC_OK;
}

}  // namespace

extern "C" {

int melspec_resample_geometry(uint32_t rate_in, uint32_t rate_out, uint32_t *orig, uint32_t *new_rate, uint32_t *width, uint32_t *max_inside_taps) {
    RsGeom g;
    if (int rc = rs_geometry(rate_in, rate_out, g)) return rs_status(rc);
    if (orig) *orig = g.orig;
    if (new_rate) *new_rate = g.nw;
    if (width) *width = g.width;
    if (max_inside_taps) *max_inside_taps = g.taps;
    return MELSPEC_OK;
}

int melspec_resample_taps(uint32_t rate_in, uint32_t rate_out, double *taps, size_t capacity) {
    RsGeom g;
    if (int rc = rs_geometry(rate_in, rate_out, g)) return rs_status(rc);
    if (!taps) return fail(MELSPEC_ERR_INVALID_ARG, "taps is NULL");
    if (capacity < static_cast<size_t>(g.nw) * g.K) return fail(MELSPEC_ERR_CAPACITY, "taps holds fewer than new * K values");
    rs_dense_taps(g, taps);
    return MELSPEC_OK;
}

size_t melspec_resample_out_len(uint32_t rate_in, uint32_t rate_out, size_t n_in) {
    if (rate_in == 0 || rate_out == 0) return 0;
    const uint32_t d = rs_gcd(rate_in, rate_out);
    return static_cast<size_t>(rs_out_len(rate_in / d, rate_out / d, n_in));
}

int melspec_resampler_create(melspec_resampler **out, int device, uint32_t rate_in, uint32_t rate_out) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    RsGeom g;
    if (int rc = rs_geometry(rate_in, rate_out, g)) return rs_status(rc);
    DeviceInfo info;
    if (int rc = pick_device(device, info)) return rc;
    melspec_resampler *r = new (std::nothrow) melspec_resampler();
    if (!r) return fail(MELSPEC_ERR_INTERNAL, "out of memory");
    auto bail = [r](int rc) { melspec_resampler_destroy(r); return rc; };
    r->dev = info; r->g = g; r->l = rs_launch(g);
    if (hipSetDevice(info.device) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipSetDevice failed"));
    if (hipStreamCreate(&r->stream) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipStreamCreate failed"));
    if (!g.copy) {
        const RsTable tb = rs_table(g);
        if (int rc = upload(r->d_win, tb.win)) return bail(rc);
        if (int rc = upload(r->d_start, tb.start)) return bail(rc);
    }
    *out = r;
    return MELSPEC_OK;
}

void melspec_resampler_destroy(melspec_resampler *r) {
    if (!r) return;
    if (r->dev.device >= 0 && hipSetDevice(r->dev.device) == hipSuccess) {
        if (r->stream) { (void)hipStreamSynchronize(r->stream); }
        r->ring.release();
        r->d_win.release(); r->d_start.release(); r->h2d.release(); r->d2h.release();
        if (r->stream) (void)hipStreamDestroy(r->stream);
    }
    delete r;
}

const char *melspec_resampler_kernel_name(const melspec_resampler *r) {
    if (!r) return "";
    switch (r->l.mode) {
        case kRsLdsAll: return "resample_kernel<lds samples, lds taps>";
        case kRsLdsSamples: return "resample_kernel<lds samples, global taps>";
        case kRsGlobal: return "resample_kernel<global samples, global taps>";
        default: return "resample_kernel<copy>";
    }
}

int melspec_resample_uniform_device(melspec_resampler *r, const void *d_pcm, int pcm_dtype, uint64_t clip_stride, uint64_t clip_len, uint32_t n_clips,
                                    float *d_out, uint64_t out_stride, void *stream) {
    if (!r) return fail(MELSPEC_ERR_INVALID_ARG, "resampler is NULL");
    if (!rs_dtype_known(pcm_dtype)) return fail(MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16");
    if (n_clips == 0 || clip_len == 0) return MELSPEC_OK;
    if (!d_pcm || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "d_pcm/d_out is NULL");
    if (rs_misaligned(d_pcm, pcm_dtype, d_out)) return fail(MELSPEC_ERR_INVALID_ARG, "d_pcm/d_out is not aligned to its element type");
    if (out_stride < rs_out_len(r->g.orig, r->g.nw, clip_len)) return fail(MELSPEC_ERR_INVALID_ARG, "out_stride is below the clips' output length");
    return rs_run(r, d_pcm, pcm_dtype, nullptr, nullptr, nullptr, clip_stride, clip_len, out_stride, n_clips, d_out, stream ? static_cast<hipStream_t>(stream) : r->stream);
}

int melspec_resample_ragged_device(melspec_resampler *r, const void *d_pcm, int pcm_dtype, const uint64_t *h_offsets, const uint64_t *h_lengths, uint32_t n_clips,
                                   float *d_out, const uint64_t *h_out_offsets, void *stream) {
    if (!r) return fail(MELSPEC_ERR_INVALID_ARG, "resampler is NULL");
    if (!rs_dtype_known(pcm_dtype)) return fail(MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16");
    if (n_clips == 0) return MELSPEC_OK;
    if (!h_offsets || !h_lengths) return fail(MELSPEC_ERR_INVALID_ARG, "offset/length array is NULL");
    if (!d_pcm || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "d_pcm/d_out is NULL");
    if (rs_misaligned(d_pcm, pcm_dtype, d_out)) return fail(MELSPEC_ERR_INVALID_ARG, "d_pcm/d_out is not aligned to its element type");
    return rs_run(r, d_pcm, pcm_dtype, h_offsets, h_lengths, h_out_offsets, 0, 0, 0, n_clips, d_out, stream ? static_cast<hipStream_t>(stream) : r->stream);
}

int melspec_resample_host(melspec_resampler *r, const void *samples, int pcm_dtype, size_t n_samples, float *out, size_t out_capacity, size_t *n_out) {
    if (!r) return fail(MELSPEC_ERR_INVALID_ARG, "resampler is NULL");
    if (!rs_dtype_known(pcm_dtype)) return fail(MELSPEC_ERR_INVALID_ARG, "pcm_dtype must be MELSPEC_PCM_F32 or MELSPEC_PCM_S16");
    if (n_samples == 0) { if (n_out) *n_out = 0; return MELSPEC_OK; }
    if (!samples || !out) return fail(MELSPEC_ERR_INVALID_ARG, "samples/out is NULL");
    if (rs_misaligned(samples, pcm_dtype, out)) return fail(MELSPEC_ERR_INVALID_ARG, "samples/out is not aligned to its element type");
    const uint64_t need = rs_out_len(r->g.orig, r->g.nw, n_samples);
    const uint64_t len = n_samples;
    const int rc = host_one_clip(r->dev.device, r->h2d, r->d2h, r->stream, samples, n_samples * (pcm_dtype == MELSPEC_PCM_S16 ? 2 : 4), out, out_capacity, need, sizeof(float),
                                 [&](void *d_in, void *d_out) { return rs_run(r, d_in, pcm_dtype, nullptr, nullptr, nullptr, len, len, need, 1, static_cast<float *>(d_out), r->stream); });
    if (rc == MELSPEC_OK && n_out) *n_out = static_cast<size_t>(need);
    return rc;
}

int melspec_resampler_synchronize(melspec_resampler *r, void *stream) {
    if (!r) return fail(MELSPEC_ERR_INVALID_ARG, "resampler is NULL");
    HIP_TRY(hipSetDevice(r->dev.device));
    HIP_TRY(hipStreamSynchronize(stream ? static_cast<hipStream_t>(stream) : r->stream));
    return MELSPEC_OK;
}

}  // extern "C"
