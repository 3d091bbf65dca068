// aux.hip -- everything around the path: the batch planners, the stand-alone mel stage and SparseMelFilterbank helpers, the streaming bank
// (src/stft.rs:48-86, src/rb.rs:86-121), the TGA quantiser (src/quant.rs), the VAD column stencil (src/vad.rs:373-415), synthetic PCM.
#include "host_common.hpp"
#include "aux_kernels.hpp"
#include "blm_stats_plan.hpp"
#include "stream_bank.hpp"
#include "mel_bank.hpp"
#include "tga_quant.hpp"
#include "vad_columns.hpp"

namespace melspec {
namespace host {

// Tables of the generic (f64 DFT) kernel.
// The banded filterbank as JOBS for the wave kernels' mel phase (pow2_frame_kernel, mel_stage_jobs_kernel): eight consecutive weights
// of one mel per job (the last job of a band padded with zeros), dealt over the rounds as described below; lf = lanes that share a
// frame (a round = lf jobs).  jobv[j] = first bin | mel << 12 | count << 20; jwv: weight pairs (2 q, 2 q + 1) of job j at [q][j].
void build_mel_jobs(const BandedFilterbank &fb, int n_mels, int lf, std::vector<double> &jwv, std::vector<int> &jobv) {
    // A job = eight consecutive bins FROM AN EVEN ONE (its eight powers are four aligned 16-byte LDS reads) with the weights of one mel
    // on them, zero where the band is not; record = first bin | mel << 12 | count << 20 (count > 0: a real job).
    struct Job { int bin, mel, lo, hi; };                    // weights of band entries [lo, hi) sit at bins bin + (entry - lo) + lead
    std::vector<Job> jobs;
    std::vector<int> lead;                                   // zero weights in front of a job's first entry
    for (int m = 0; m < n_mels && m < 256; ++m) {
        const int st = fb.start[m], len = fb.len[m];
        if (len <= 0) continue;
        for (int b = st & ~1; b < st + len; b += 8) {
            const int lo = std::max(b, st) - st, hi = std::min(b + 8, st + len) - st;
            jobs.push_back({b, m, lo, hi});
            lead.push_back(std::max(b, st) - b);
        }
    }
#ifndef MS_POW2_JOBORDER
#define MS_POW2_JOBORDER 1
#endif
    // The lanes of a round read their jobs' powers with ds_read_b128, which the LDS serves in groups of sixteen lanes -- {0-3, 12-15,
    // 20-27}, {4-11, 16-19, 28-31} and the same + 32 -- over the sixteen 16-byte slots of a 256-byte row: the jobs that meet in such a
    // group want first bins whose halves differ mod 16 (mod 8 where a frame has eight lanes: the group then holds the same eight jobs
    // of two pairs of frames, whose rows pow2_pw_shift sets eight slots apart).  In band order they do not -- a band's jobs are 8 bins
    // apart, the low bands 2-3 -- and the reads were 3-4-way (SQ_LDS_BANK_CONFLICT: 25 % of the LDS cycles at n_fft 2048).  So: sets of
    // g jobs; a job with fewer than eight entries may start 2, 4 or 6 bins early (more zeros in front); every job goes to the set that
    // holds the fewest jobs of its residue (then of its mel: ds_add_f64 to one address serialises), fullest residue classes first;
    // the sets padded with empty jobs (count 0) and laid onto the lane groups.  The order is a function of the bank: the sums stay
    // deterministic; a band's pieces are added in another order than the reference's left fold (f64: ~1e-16 relative).
    const int g = lf >= 16 ? 16 : 8;
    const size_t nj = jobs.size(), sets = std::max<size_t>(1, (nj + g - 1) / g);
    std::vector<std::vector<size_t>> grp(sets);
    std::vector<int> shift(nj, 0);
    if (MS_POW2_JOBORDER && lf >= 8) {
        std::vector<std::vector<size_t>> cls(g);
        for (size_t j = 0; j < nj; ++j) cls[(jobs[j].bin >> 1) % g].push_back(j);
        std::vector<int> order(g);
        for (int r = 0; r < g; ++r) order[r] = r;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return cls[x].size() > cls[y].size(); });
        std::vector<std::vector<int>> used(sets, std::vector<int>(g, 0));
        for (int r : order)
            for (size_t j : cls[r]) {
                size_t best = sets;
                int best_shift = 0;
                long best_key = 0;
                const int room = 8 - (lead[j] + (jobs[j].hi - jobs[j].lo));
                for (int sh = 0; sh <= room && sh <= jobs[j].bin; sh += 2) {
                    const int res = ((jobs[j].bin - sh) >> 1) % g;
                    for (size_t q = 0; q < sets; ++q) {
                        if (grp[q].size() >= static_cast<size_t>(g)) continue;
                        long same_mel = 0;
                        for (size_t o : grp[q]) same_mel += jobs[o].mel == jobs[j].mel;
                        const long key = (static_cast<long>(used[q][res]) << 40) + (same_mel << 24) + (static_cast<long>(sh) << 16) + static_cast<long>(grp[q].size());
                        if (best == sets || key < best_key) { best = q; best_key = key; best_shift = sh; }
                    }
                }
                grp[best].push_back(j);
                shift[j] = best_shift;
                used[best][((jobs[j].bin - best_shift) >> 1) % g] += 1;
            }
    } else {
        for (size_t j = 0; j < nj; ++j) grp[j / g].push_back(j);
    }
    // lane positions: lf >= 32: two sets per 32 lanes, on the two lane groups of ds_read_b128; else a set = the lanes of a frame
    static const int kLanesOfGroup[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27}, {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
    const size_t slots = lf >= 32 ? ((sets + 1) / 2) * 32 : sets * g;
    std::vector<long> at(slots, -1);
    for (size_t q = 0; q < sets; ++q) {
        std::sort(grp[q].begin(), grp[q].end());
        for (size_t i = 0; i < grp[q].size(); ++i)
            at[lf >= 32 ? (q / 2) * 32 + kLanesOfGroup[q & 1][i] : q * g + i] = static_cast<long>(grp[q][i]);
    }
    jobv.assign(nj ? slots : 1, 0);
    std::vector<double> w8((nj ? slots : 1) * 8, 0.0);
    for (size_t pos = 0; pos < slots && nj; ++pos) {
        if (at[pos] < 0) continue;
        const size_t j = static_cast<size_t>(at[pos]);
        const Job &jb = jobs[j];
        const int bin = jb.bin - shift[j], first = lead[j] + shift[j];
        jobv[pos] = bin | (jb.mel << 12) | ((jb.hi - jb.lo) << 20);
        for (int e = jb.lo; e < jb.hi; ++e) w8[8 * pos + first + (e - jb.lo)] = fb.w[static_cast<size_t>(fb.offset[jb.mel]) + e];
    }
    // weight pairs (2 q, 2 q + 1) of the job at position j at [q][j]: the lanes of a round read consecutive 16-byte slots
    const size_t np = jobv.size();
    jwv.assign(8 * np, 0.0);
    for (size_t j = 0; j < np; ++j)
        for (int q = 0; q < 8; ++q) jwv[2 * ((q / 2) * np + j) + (q & 1)] = w8[8 * j + q];
}

__global__ void plan_upload_kernel(const uint4 *src, uint4 *dst, size_t n16) {
    for (size_t i = blockIdx.x * static_cast<size_t>(blockDim.x) + threadIdx.x; i < n16; i += static_cast<size_t>(gridDim.x) * blockDim.x) dst[i] = src[i];
}

// Fills the next slot and queues its upload on `stream`.  The caller launches on `stream` and then calls plan_ragged_done.
// want_order: also upload the clips sorted longest first and a zeroed ticket counter (BatchDesc::d_order / d_ticket) for the kernels that
// hand out whole clips.
int plan_ragged(RaggedScratch &rs, hipStream_t stream, const float *d_pcm, float *d_out, const uint64_t *h_off,
                const std::vector<uint64_t> &frames, const uint64_t *h_out_off, uint32_t n_clips, int n_mels,
                int frames_per_unit, BatchPlan &pl, RaggedSlot *&used, bool want_order, uint32_t round_units) {
    // round_units (1: as they are): every clip's units rounded up to a multiple of it -- the split output's kernels want whole rounds of
    // their workgroup per clip (blm_stats_plan.hpp); the units past a clip's frames compute and store nothing
    const auto units_of = [&](uint64_t fr) { return ragged_clip_units(fr, static_cast<uint32_t>(frames_per_unit), round_units); };
    uint64_t units = 0;
    for (uint32_t c = 0; c < n_clips; ++c) units += units_of(frames[c]);
    const uint64_t n_blocks = (units + kUnitBlock - 1) / kUnitBlock;
    const size_t words64 = static_cast<size_t>(n_clips) * 4 + 1;
    const size_t blk_words = static_cast<size_t>(n_blocks ? n_blocks : 1);
    const size_t bytes = round16(words64 * sizeof(uint64_t) + (blk_words + (want_order ? static_cast<size_t>(n_clips) + 1 : 0)) * sizeof(uint32_t));
    if (int rc = table_slot_take(rs, bytes, used)) return rc;
    RaggedSlot &sl = *used;
    uint64_t *off = static_cast<uint64_t *>(sl.host), *fr = off + n_clips, *oo = fr + n_clips, *pre = oo + n_clips;
    uint32_t *blk = reinterpret_cast<uint32_t *>(off + words64);
    uint64_t cursor = 0, out_cursor = 0, total = 0;
    for (uint32_t c = 0; c < n_clips; ++c) {
        off[c] = h_off[c];
        fr[c] = frames[c];
        oo[c] = h_out_off ? h_out_off[c] : out_cursor;
        out_cursor += frames[c] * static_cast<uint64_t>(n_mels);
        pre[c] = cursor;
        cursor += units_of(frames[c]);
        total += frames[c];
    }
    pre[n_clips] = units;
    {
        uint32_t c = 0;
        for (uint64_t k = 0; k < n_blocks; ++k) {
            const uint64_t u = k * kUnitBlock;
            while (pre[c + 1] <= u) ++c;      // u < units = pre[n_clips]
            blk[k] = c;
        }
    }
    if (want_order) {
        uint32_t *ord = blk + blk_words;
        for (uint32_t c = 0; c < n_clips; ++c) ord[c] = c;
        std::stable_sort(ord, ord + n_clips, [&](uint32_t a, uint32_t b2) { return frames[a] > frames[b2]; });
        // the order ends at the last clip with a frame: the clips without one sort to the end, and a ticket past the end reads "the batch is
        // used up" (fbank512_clip_kernel's clip_queue_get) -- a wave that could skip clips without arriving for them would break the bound
        // its ring of clip ids relies on
        for (uint32_t i = n_clips; i > 0 && frames[ord[i - 1]] == 0; --i) ord[i - 1] = 0xffffffffu;
        ord[n_clips] = 0;       // the ticket counter
    }
    if (int rc = table_slot_upload(sl, bytes, stream)) return rc;
    const uint64_t *d = static_cast<const uint64_t *>(sl.dev.p);
    BatchDesc &b = pl.desc;
    b = BatchDesc{};
    b.pcm = d_pcm; b.out = d_out; b.n_clips = n_clips; b.n_units = units; b.frames_per_unit = frames_per_unit;
    b.d_off = d; b.d_frames = d + n_clips; b.d_out_off = d + 2 * n_clips; b.d_unit_prefix = d + 3 * n_clips;
    b.d_unit_block = reinterpret_cast<const uint32_t *>(d + words64);
    if (want_order) {
        b.d_order = b.d_unit_block + blk_words;
        b.d_ticket = const_cast<uint32_t *>(b.d_order) + n_clips;
    }
    pl.total_frames = total;
    b.stat_frames = total;
    return MELSPEC_OK;
}
// behind the launch (or the failed attempt) that used the slot
void plan_ragged_done(RaggedSlot *sl, hipStream_t stream) {
    if (sl && sl->ev && hipEventRecord(sl->ev, stream) == hipSuccess) sl->pending = true;
}

// ---- a table's trip to the device through a ring slot (the ragged plans above, the stream banks' entries: stream_bank.hpp), and the banks'
// scatter / carry kernels (geometry-agnostic: they read the slot stride, in_off and the entries) ----
// the next slot of the ring with room for `bytes` (a multiple of 16) on both sides; the caller fills sl->host, then table_slot_upload
int table_slot_take(RaggedScratch &ring, size_t bytes, RaggedSlot *&sl) {
    sl = &ring.slot[ring.next++ % RaggedScratch::kSlots];
    if (!sl->ev) HIP_TRY(hipEventCreateWithFlags(&sl->ev, hipEventDisableTiming));
    if (sl->pending) { HIP_TRY(hipEventSynchronize(sl->ev)); sl->pending = false; }
    if (int rc = sl->ensure_host(bytes)) return rc;
    return sl->dev.ensure(bytes);
}
// the upload is a kernel on the launch stream that reads the pinned slot over the bus: an SDMA copy sits in another hardware queue and the
// hand-over between the queues costs more than the copy.  Afterwards the slot is in use until plan_ragged_done's event
int table_slot_upload(RaggedSlot &sl, size_t bytes, hipStream_t s) {
    const size_t n16 = bytes / 16;
    const unsigned blocks = static_cast<unsigned>((n16 + 255) / 256 < 1024 ? (n16 + 255) / 256 : 1024);
    hipLaunchKernelGGL(plan_upload_kernel, dim3(blocks ? blocks : 1), dim3(256), 0, s, static_cast<const uint4 *>(sl.host), static_cast<uint4 *>(sl.dev.p), n16);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}
int stream_scatter_launch(float *state, uint64_t stride, uint32_t in_off, const StreamEntry *d_e, uint32_t n, const void *d_src, int pcm_dtype, hipStream_t s) {
    if (pcm_dtype == MELSPEC_PCM_S16)
        hipLaunchKernelGGL(stream_scatter_kernel<io_s16>, dim3(n), dim3(256), 0, s, state, stride, in_off, d_e, static_cast<const io_s16 *>(d_src));
    else
        hipLaunchKernelGGL(stream_scatter_kernel<float>, dim3(n), dim3(256), 0, s, state, stride, in_off, d_e, static_cast<const float *>(d_src));
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}
int stream_carry_launch(float *state, uint64_t stride, uint32_t in_off, const StreamEntry *d_e, uint32_t n, hipStream_t s) {
    hipLaunchKernelGGL(stream_carry_kernel, dim3(n), dim3(256), 0, s, state, stride, in_off, d_e);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int plan_ragged_device(DevicePlan &dp, hipStream_t stream, const float *d_pcm, float *d_out, const uint64_t *d_off, const uint64_t *d_len,
                       const uint64_t *d_out_off, uint32_t n_clips, uint64_t frame_len, uint64_t frame_shift, uint32_t words_per_frame,
                       int frames_per_unit, uint64_t max_total_frames, BatchPlan &pl) {
    // every clip with frames has at most frames / fpu + 1 units
    const uint64_t max_units = max_total_frames / frames_per_unit + n_clips;
    const uint64_t max_blocks = max_units / kUnitBlock + 2;
    const size_t words64 = static_cast<size_t>(n_clips) * 4 + 1;
    const size_t bytes = words64 * sizeof(uint64_t) + static_cast<size_t>(max_blocks) * sizeof(uint32_t) + 16;
    if (dp.used && dp.last != stream) HIP_TRY(hipStreamSynchronize(dp.last));
    if (bytes > dp.buf.cap && dp.used) HIP_TRY(hipStreamSynchronize(dp.last));
    int rc = dp.buf.ensure(bytes);
    if (rc) return rc;
    dp.used = true; dp.last = stream;
    PlanParams q{};
    q.d_off = d_off; q.d_len = d_len; q.d_out_off = d_out_off; q.n_clips = n_clips;
    q.frame_len = frame_len; q.frame_shift = frame_shift; q.words_per_frame = words_per_frame;
    q.frames_per_unit = static_cast<uint32_t>(frames_per_unit);
    q.plan = static_cast<uint64_t *>(dp.buf.p);
    q.max_blocks = max_blocks;
    hipLaunchKernelGGL(plan_ragged_device_kernel, dim3(1), dim3(1024), 0, stream, q);
    HIP_TRY(hipGetLastError());
    const uint64_t *d = q.plan;
    BatchDesc &b = pl.desc;
    b = BatchDesc{};
    b.pcm = d_pcm; b.out = d_out; b.n_clips = n_clips; b.n_units = max_units; b.frames_per_unit = frames_per_unit;
    b.d_off = d; b.d_frames = d + n_clips; b.d_out_off = d + 2 * n_clips; b.d_unit_prefix = d + 3 * n_clips;
    b.d_unit_block = reinterpret_cast<const uint32_t *>(d + words64);
    b.d_n_units = d + 4 * static_cast<size_t>(n_clips);        // prefix[n_clips]
    pl.total_frames = max_total_frames;
    return MELSPEC_OK;
}

int blm_plan_ragged_device(DevicePlan &dp, hipStream_t stream, const float *d_pcm, float *d_out, const uint64_t *d_off, const uint64_t *d_len,
                           const uint64_t *d_out_off, uint32_t n_clips, const BlmDescGeom &geom, uint64_t max_total_columns, uint64_t max_clip_samples,
                           uint32_t *d_rejected, BatchPlan &pl, BlmDevicePlanAux &aux) {
    const uint64_t max_units = blm_desc_max_units(max_total_columns, n_clips);
    const uint64_t max_blocks = blm_desc_max_blocks(max_units);
    const size_t bytes = blm_desc_bytes(n_clips, max_blocks);
    if (dp.used && dp.last != stream) HIP_TRY(hipStreamSynchronize(dp.last));
    if (bytes > dp.buf.cap && dp.used) HIP_TRY(hipStreamSynchronize(dp.last));
    int rc = dp.buf.ensure(bytes);
    if (rc) return rc;
    dp.used = true; dp.last = stream;
    BlmPlanParams q{};
    q.d_off = d_off; q.d_len = d_len; q.d_out_off = d_out_off; q.n_clips = n_clips;
    q.geom = geom;
    q.max_total_columns = max_total_columns; q.max_clip_samples = max_clip_samples;
    q.plan = static_cast<uint64_t *>(dp.buf.p);
    q.max_blocks = max_blocks;
    q.d_rejected = d_rejected;
    hipLaunchKernelGGL(blm_plan_ragged_device_kernel, dim3(1), dim3(1024), 0, stream, q);
    HIP_TRY(hipGetLastError());
    const BlmDescTables t = blm_desc_tables(q.plan, n_clips);
    BatchDesc &b = pl.desc;
    b = BatchDesc{};
    b.pcm = d_pcm; b.out = d_out; b.n_clips = n_clips; b.n_units = max_units; b.frames_per_unit = static_cast<int>(kBlmDescFramesPerUnit);
    b.d_off = t.off; b.d_frames = t.frames; b.d_out_off = t.out_off; b.d_unit_prefix = t.prefix;
    b.d_unit_block = t.blk;
    b.d_n_units = t.prefix + n_clips;
    pl.total_frames = max_total_columns;
    aux.d_len = t.len; aux.d_valid = t.valid; aux.d_ctr = t.ctr; aux.d_order = t.order;
    return MELSPEC_OK;
}

}  // namespace host
}  // namespace melspec

extern "C" {

// ---- the mel stage on its own: MelSpectrogram::add(&fft) (src/mel.rs:13-32) over complex STFT frames --------------------------
namespace {
int stage_tables(melspec_ctx *c) {
    if (c->stage_built) return MELSPEC_OK;
    const int bins = c->fft_size / 2 + 1;
    const BandedFilterbank fb = band_filterbank(c->dense, c->n_mels, bins, c->fft_size / 2);      // bins >= n_fft/2 contribute nothing (src/mel.rs:155-163)
    int rc;
    if ((rc = upload(c->st_start, fb.start))) return rc;
    if ((rc = upload(c->st_len, fb.len))) return rc;
    if ((rc = upload(c->st_off, fb.offset))) return rc;
    if ((rc = upload(c->st_w, fb.w))) return rc;
    {
        std::vector<double> jwv;
        std::vector<int> jobv;
        build_mel_jobs(fb, c->n_mels, 64, jwv, jobv);
        c->st_n_jobs = jobv.size() == 1 && (jobv[0] >> 20) == 0 ? 0 : static_cast<int>(jobv.size());
        if ((rc = upload(c->st_jw, jwv))) return rc;
        if ((rc = upload(c->st_job, jobv))) return rc;
    }
    c->stage_built = true;
    return MELSPEC_OK;
}
}  // namespace

int melspec_mel_from_stft_device(melspec_ctx *c, const void *d_spec, int dtype, int full, uint64_t n_frames, float *d_out, void *stream) {
    if (!c) return fail(MELSPEC_ERR_INVALID_ARG, "ctx is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_frames == 0) return MELSPEC_OK;
    if (!d_spec || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    HIP_TRY(hipSetDevice(c->dev.device));
    int rc = stage_tables(c);
    if (rc) return rc;
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    MelStageParams p{};
    p.spec = d_spec; p.out = d_out; p.n_frames = n_frames;
    p.stride = static_cast<uint32_t>(full ? c->fft_size : c->fft_size / 2 + 1);
    p.bin_limit = c->fft_size / 2; p.n_mels = c->n_mels;
    p.d_mstart = static_cast<const int *>(c->st_start.p); p.d_mlen = static_cast<const int *>(c->st_len.p);
    p.d_moff = static_cast<const int *>(c->st_off.p); p.d_mw = static_cast<const double *>(c->st_w.p);
    p.d_jw = static_cast<const double *>(c->st_jw.p); p.d_job = static_cast<const int *>(c->st_job.p); p.n_jobs = c->st_n_jobs;
    {
        // the wave-per-frame form with the bank as jobs in LDS (banks of up to 256 mels over up to 4088 bins that fit)
        const size_t lds = sizeof(double) * static_cast<size_t>(mel_stage_lds(p.n_jobs, p.bin_limit, p.n_mels, kMelStageWaves).total);
        if (p.n_jobs > 0 && p.n_mels <= 256 && p.bin_limit <= 4088 && lds <= 64 * 1024) {
            const unsigned grid = grid_for((n_frames + kMelStageWaves - 1) / kMelStageWaves, c->dev.cus, static_cast<int>(std::max<size_t>(1, std::min<size_t>(4, kLdsLimit / lds))));
            if (dtype == MELSPEC_STFT_F64) hipLaunchKernelGGL((mel_stage_jobs_kernel<double>), dim3(grid), dim3(kMelStageWaves * 64), lds, s, p);
            else hipLaunchKernelGGL((mel_stage_jobs_kernel<float>), dim3(grid), dim3(kMelStageWaves * 64), lds, s, p);
            HIP_TRY(hipGetLastError());
            return MELSPEC_OK;
        }
    }
    constexpr int kWaves = 4;
    const size_t lds = static_cast<size_t>(kWaves) * (p.bin_limit + p.n_mels) * sizeof(double);
    if (lds > 64 * 1024) return fail(MELSPEC_ERR_UNSUPPORTED, "geometry needs more LDS than the mel stage kernel has");
    const unsigned grid = grid_for((n_frames + kWaves - 1) / kWaves, c->dev.cus, 16);
    if (dtype == MELSPEC_STFT_F64) hipLaunchKernelGGL((mel_stage_kernel<double, kWaves>), dim3(grid), dim3(kWaves * 64), lds, s, p);
    else hipLaunchKernelGGL((mel_stage_kernel<float, kWaves>), dim3(grid), dim3(kWaves * 64), lds, s, p);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_mel_from_stft_host(melspec_ctx *c, const void *spec, int dtype, int full, size_t n_frames, float *out, size_t out_capacity_floats) {
    if (!c) return fail(MELSPEC_ERR_INVALID_ARG, "ctx is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_frames == 0) return MELSPEC_OK;
    if (!spec || !out) return fail(MELSPEC_ERR_INVALID_ARG, "spec/out is NULL");
    const size_t need = n_frames * static_cast<size_t>(c->n_mels);
    if (out_capacity_floats < need) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
    HIP_TRY(hipSetDevice(c->dev.device));
    const size_t in_bytes = n_frames * static_cast<size_t>(full ? c->fft_size : c->fft_size / 2 + 1) * 2 * (dtype == MELSPEC_STFT_F64 ? sizeof(double) : sizeof(float));
    void *d_in = nullptr, *d_o = nullptr;
    HIP_TRY(hipMalloc(&d_in, in_bytes));
    hipError_t e = hipMalloc(&d_o, need * sizeof(float));
    if (e != hipSuccess) { (void)hipFree(d_in); return fail_hip(e, "hipMalloc"); }
    int rc = MELSPEC_OK;
    if ((e = hipMemcpyAsync(d_in, spec, in_bytes, hipMemcpyHostToDevice, c->stream)) != hipSuccess) rc = fail_hip(e, "hipMemcpyAsync");
    if (!rc) rc = melspec_mel_from_stft_device(c, d_in, dtype, full, n_frames, static_cast<float *>(d_o), c->stream);
    if (!rc && (e = hipMemcpyAsync(out, d_o, need * sizeof(float), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) rc = fail_hip(e, "hipMemcpyAsync");
    if ((e = hipStreamSynchronize(c->stream)) != hipSuccess && !rc) rc = fail_hip(e, "hipStreamSynchronize");
    (void)hipFree(d_in); (void)hipFree(d_o);
    return rc;
}

}  // extern "C"

// ---- stand-alone mel helpers (mel_bank.hpp): SparseMelFilterbank, project_power, log_mel_spectrogram, norm_mel -------------------
struct melspec_bank {
    DeviceInfo dev;
    hipStream_t stream = nullptr;
    int n_mels = 0, fft_bins = 0, nnz = 0;
    DevBuf row_ptr, bin, w, wf, key, tmp_in, tmp_out;
    hipStream_t key_stream = nullptr;              // norm_mel's scratch word is used in stream order: a call on another stream first waits for this one
    bool key_used = false;
    std::vector<int> h_row_ptr, h_bin;             // the sparse rows on the host (weights_for_mel)
    std::vector<double> h_w;
    BankDesc desc() const {
        return BankDesc{static_cast<const int *>(row_ptr.p), static_cast<const int *>(bin.p), static_cast<const double *>(w.p),
                        static_cast<const float *>(wf.p), n_mels, fft_bins};
    }
};

namespace {
int bank_create(melspec_bank **out, int device, const std::vector<double> &dense, int n_mels, int fft_bins) {
    DeviceInfo info;
    int rc = pick_device(device, info);
    if (rc) return rc;
    melspec_bank *b = new (std::nothrow) melspec_bank();
    if (!b) return fail(MELSPEC_ERR_INTERNAL, "out of host memory");
    b->dev = info; b->n_mels = n_mels; b->fft_bins = fft_bins;
    auto bail = [&](int code) { melspec_bank_destroy(b); return code; };
    if (hipSetDevice(info.device) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipSetDevice failed"));
    if (hipStreamCreate(&b->stream) != hipSuccess) return bail(fail(MELSPEC_ERR_UNAVAILABLE, "hipStreamCreate failed"));
    // from_dense (src/mel.rs:48-71): per row the non-zero entries in ascending bin order
    std::vector<int> row_ptr(static_cast<size_t>(n_mels) + 1, 0), bins;
    std::vector<double> w;
    std::vector<float> wf;
    for (int m = 0; m < n_mels; ++m) {
        for (int k = 0; k < fft_bins; ++k) {
            const double v = dense[static_cast<size_t>(m) * fft_bins + k];
            if (v != 0.0) { bins.push_back(k); w.push_back(v); wf.push_back(static_cast<float>(v)); }
        }
        row_ptr[m + 1] = static_cast<int>(bins.size());
    }
    b->nnz = static_cast<int>(bins.size());
    b->h_row_ptr = row_ptr; b->h_bin = bins; b->h_w = w;
    if ((rc = upload(b->row_ptr, row_ptr)) || (rc = upload(b->bin, bins)) || (rc = upload(b->w, w)) || (rc = upload(b->wf, wf))) return bail(rc);
    if ((rc = b->key.ensure(16))) return bail(rc);
    *out = b;
    return MELSPEC_OK;
}

template <class T>
int norm_launch(const T *d_in, uint64_t n, T *d_out, unsigned long long *key, int cus, hipStream_t s) {
    const unsigned grid = static_cast<unsigned>(std::min<uint64_t>((n + 255) / 256, static_cast<uint64_t>(cus) * 16));
    hipLaunchKernelGGL(norm_init_kernel, dim3(1), dim3(1), 0, s, key);
    hipLaunchKernelGGL(norm_max_kernel<T>, dim3(grid), dim3(256), 0, s, d_in, n, key);
    hipLaunchKernelGGL(norm_map_kernel<T>, dim3(grid), dim3(256), 0, s, d_in, n, key, d_out);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}
}  // namespace

extern "C" {

int melspec_bank_from_dense(melspec_bank **out, int device, const double *filters, int n_mels, int fft_bins) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!filters || n_mels <= 0 || fft_bins <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "filters is NULL or a dimension is not positive");
    return bank_create(out, device, std::vector<double>(filters, filters + static_cast<size_t>(n_mels) * fft_bins), n_mels, fft_bins);
}

int melspec_bank_from_mel(melspec_bank **out, int device, double sample_rate, int n_fft, int n_mels, double f_min, double f_max, int htk, int norm) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!(sample_rate > 0.0) || n_fft < 2 || n_mels <= 0) return fail(MELSPEC_ERR_INVALID_ARG, "sample_rate, n_fft and n_mels must be positive");
    return bank_create(out, device, mel_filterbank(sample_rate, n_fft, n_mels, f_min, f_max, htk != 0, norm != 0), n_mels, n_fft / 2 + 1);
}

void melspec_bank_destroy(melspec_bank *b) {
    if (!b) return;
    if (b->dev.device >= 0) (void)hipSetDevice(b->dev.device);
    if (b->stream) { (void)hipStreamSynchronize(b->stream); (void)hipStreamDestroy(b->stream); }
    b->row_ptr.release(); b->bin.release(); b->w.release(); b->wf.release(); b->key.release(); b->tmp_in.release(); b->tmp_out.release();
    delete b;
}

int melspec_bank_n_mels(const melspec_bank *b) { return b ? b->n_mels : 0; }
int melspec_bank_fft_bins(const melspec_bank *b) { return b ? b->fft_bins : 0; }
int melspec_bank_non_zero_weights(const melspec_bank *b) { return b ? b->nnz : 0; }

int melspec_bank_weights_for_mel(const melspec_bank *b, int mel_idx, int *bins, double *weights, int capacity) {
    if (!b || mel_idx < 0 || mel_idx >= b->n_mels) return -1;
    const int lo = b->h_row_ptr[mel_idx], n = b->h_row_ptr[mel_idx + 1] - lo;
    for (int i = 0; i < n && i < capacity; ++i) {
        if (bins) bins[i] = b->h_bin[lo + i];
        if (weights) weights[i] = b->h_w[lo + i];
    }
    return n;
}

int melspec_bank_project_power_device(melspec_bank *b, const void *d_power, int dtype, uint64_t n_frames, void *d_out, void *stream) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "bank is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_frames == 0) return MELSPEC_OK;
    if (!d_power || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    const uint64_t items = n_frames * static_cast<uint64_t>(b->n_mels);
    if ((items + 255) / 256 > 0x7fffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "too many frames for one call");
    const dim3 grid(static_cast<unsigned>((items + 255) / 256));
    if (dtype == MELSPEC_STFT_F64)
        hipLaunchKernelGGL(bank_project_power_kernel<double>, grid, dim3(256), 0, s, b->desc(), static_cast<const double *>(d_power), static_cast<double *>(d_out), n_frames);
    else
        hipLaunchKernelGGL(bank_project_power_kernel<float>, grid, dim3(256), 0, s, b->desc(), static_cast<const float *>(d_power), static_cast<float *>(d_out), n_frames);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_bank_log_mel_device(melspec_bank *b, const void *d_stft, int dtype, int n_fft, uint64_t n_frames, double *d_out, void *stream) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "bank is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_fft < 2 || n_fft < b->fft_bins) return fail(MELSPEC_ERR_INVALID_ARG, "n_fft must be at least the bank's fft_bins");
    if (n_frames == 0) return MELSPEC_OK;
    if (!d_stft || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    const uint64_t items = n_frames * static_cast<uint64_t>(b->n_mels);
    if ((items + 255) / 256 > 0x7fffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "too many frames for one call");
    const dim3 grid(static_cast<unsigned>((items + 255) / 256));
    if (dtype == MELSPEC_STFT_F64)
        hipLaunchKernelGGL(bank_log_mel_kernel<double>, grid, dim3(256), 0, s, b->desc(), static_cast<const double *>(d_stft), n_fft, d_out, n_frames);
    else
        hipLaunchKernelGGL(bank_log_mel_kernel<float>, grid, dim3(256), 0, s, b->desc(), static_cast<const float *>(d_stft), n_fft, d_out, n_frames);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_bank_norm_mel_device(melspec_bank *b, const void *d_in, int dtype, uint64_t n_values, void *d_out, void *stream) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "bank is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_values == 0) return MELSPEC_OK;
    if (!d_in || !d_out) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    HIP_TRY(hipSetDevice(b->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : b->stream;
    unsigned long long *key = static_cast<unsigned long long *>(b->key.p);
    // the three launches of a call (init, max, map) share ONE scratch word per bank: two calls on different streams would race on it
    //  -- like FixState::last_stream, a change of stream waits for the previous one
    if (b->key_used && b->key_stream != s) HIP_TRY(hipStreamSynchronize(b->key_stream));
    b->key_used = true; b->key_stream = s;
    return dtype == MELSPEC_STFT_F64 ? norm_launch<double>(static_cast<const double *>(d_in), n_values, static_cast<double *>(d_out), key, b->dev.cus, s)
                                     : norm_launch<float>(static_cast<const float *>(d_in), n_values, static_cast<float *>(d_out), key, b->dev.cus, s);
}

// host forms: staged through the bank's own buffers, synchronous
static int bank_host_call(melspec_bank *b, const void *in, size_t in_bytes, void *out, size_t out_bytes, int (*run)(melspec_bank *, const void *, void *, void *), void *ctx) {
    HIP_TRY(hipSetDevice(b->dev.device));
    int rc;
    if ((rc = b->tmp_in.ensure(in_bytes + 16)) || (rc = b->tmp_out.ensure(out_bytes + 16))) return rc;
    HIP_TRY(hipMemcpyAsync(b->tmp_in.p, in, in_bytes, hipMemcpyHostToDevice, b->stream));
    if ((rc = run(b, b->tmp_in.p, b->tmp_out.p, ctx))) { (void)hipStreamSynchronize(b->stream); return rc; }
    HIP_TRY(hipMemcpyAsync(out, b->tmp_out.p, out_bytes, hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return MELSPEC_OK;
}

int melspec_bank_project_power_host(melspec_bank *b, const void *power, int dtype, size_t n_frames, void *out) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "bank is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_frames == 0) return MELSPEC_OK;
    if (!power || !out) return fail(MELSPEC_ERR_INVALID_ARG, "pointer is NULL");
    const size_t el = dtype == MELSPEC_STFT_F64 ? 8 : 4;
    struct A { int dtype; uint64_t n; } a{dtype, n_frames};
    return bank_host_call(b, power, n_frames * b->fft_bins * el, out, n_frames * b->n_mels * el,
                          [](melspec_bank *bb, const void *i, void *o, void *c) { auto *x = static_cast<A *>(c); return melspec_bank_project_power_device(bb, i, x->dtype, x->n, o, bb->stream); }, &a);
}

int melspec_bank_log_mel_host(melspec_bank *b, const void *stft, int dtype, int n_fft, size_t n_frames, double *out) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "bank is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_fft < 2) return fail(MELSPEC_ERR_INVALID_ARG, "n_fft must be >= 2");
    if (n_frames == 0) return MELSPEC_OK;
    if (!stft || !out) return fail(MELSPEC_ERR_INVALID_ARG, "pointer is NULL");
    const size_t el = dtype == MELSPEC_STFT_F64 ? 8 : 4;
    struct A { int dtype, n_fft; uint64_t n; } a{dtype, n_fft, n_frames};
    return bank_host_call(b, stft, n_frames * n_fft * 2 * el, out, n_frames * b->n_mels * 8,
                          [](melspec_bank *bb, const void *i, void *o, void *c) { auto *x = static_cast<A *>(c); return melspec_bank_log_mel_device(bb, i, x->dtype, x->n_fft, x->n, static_cast<double *>(o), bb->stream); }, &a);
}

int melspec_bank_norm_mel_host(melspec_bank *b, const void *in, int dtype, size_t n_values, void *out) {
    if (!b) return fail(MELSPEC_ERR_INVALID_ARG, "bank is NULL");
    if (dtype != MELSPEC_STFT_F32 && dtype != MELSPEC_STFT_F64) return fail(MELSPEC_ERR_INVALID_ARG, "dtype must be MELSPEC_STFT_F32 or MELSPEC_STFT_F64");
    if (n_values == 0) return MELSPEC_OK;
    if (!in || !out) return fail(MELSPEC_ERR_INVALID_ARG, "pointer is NULL");
    const size_t el = dtype == MELSPEC_STFT_F64 ? 8 : 4;
    struct A { int dtype; uint64_t n; } a{dtype, n_values};
    return bank_host_call(b, in, n_values * el, out, n_values * el,
                          [](melspec_bank *bb, const void *i, void *o, void *c) { auto *x = static_cast<A *>(c); return melspec_bank_norm_mel_device(bb, i, x->dtype, x->n, o, bb->stream); }, &a);
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// Streaming: a bank of live streams with device-side overlap-save state
// (Spectrogram::add src/stft.rs:48-86 driven by RingBuffer::maybe_mel src/rb.rs:86-121)
// ------------------------------------------------------------------------------------
struct melspec_stream {
    melspec_ctx *ctx = nullptr;          // geometry, tables, kernels; not owned
    StreamGeom geom{};
    StreamBook book;                     // pending / idx per stream (host side of the state)
    BankCore core;
    // the detector stage (melspec_stream_enable_vad): VoiceActivityDetector state per stream, in HBM
    bool vad_on = false;
    melspec_vad_settings vad{};
    DevBuf vad_state, vad_prev, vad_acts;
    std::vector<uint64_t> vad_count;     // host copy of StreamVadState::count (VoiceActivityDetector::frame_index)
    // The plan of the last push, and -- while `key` is valid -- its entry table and ragged plan on the device: a push that repeats it
    // (PushKey, stream_plan.hpp) builds and uploads neither again (4096 streams x 1 hop: 0.089 -> 0.05 ms per push).
    struct {
        PushKey key;
        StreamPlan pl;
        const StreamEntry *d_e = nullptr;    // the entries in the ring slot of the push that filled the key
        BatchPlan plan;
    } cache;
};

namespace {
// what a push emits per frame: the mel row (Spectrogram::add + MelSpectrogram::add) or the spectrum (Spectrogram::add alone)
struct StreamEmit {
    bool stft = false;
    int dtype = MELSPEC_STFT_F32, full = 0;
};

// one push of the bank: q.io = pcm_dtype | out_dtype << 4 (stream_io_args) -- the scatter converts the chunks into the f32 state, which
// is what the frame kernels read, so only the out half of the code reaches launch_ctx
struct StreamPush {
    PushQuery q;
    bool flush = false;
    StreamEmit emit;
    bool want_acts = false;                      // the caller takes the detector's records: the host forms', in `acts`
    melspec_vad_activity *acts = nullptr;
    size_t acts_capacity = 0;
    melspec_vad_activity *d_acts = nullptr;      // the detector's records on the device (NULL: the bank's own buffer)
    bool hit = false;                            // the push repeats the cached one: decided by stream_prepare, nowhere else
};

// The plan of the push in st->cache.pl: the one that is there if the push repeats it, else a fresh one (the key goes first: the plan it
// stood for is overwritten, and the ring slot its entries are in may be the next one taken).  A host push's q.d_out is the bank's out
// buffer: a hit ran from that buffer with as many rows, so the push finds room in it and the pointer stays.
int stream_prepare(melspec_stream *st, StreamPush &p, const uint32_t *ids, const uint32_t *lens, uint32_t n) {
    p.q.ids = ids; p.q.lens = lens; p.q.n = n; p.q.fpu = ctx_frames_per_unit(st->ctx);
    p.q.repeatable = !p.flush && !p.emit.stft;
    if ((p.hit = st->cache.key.matches(st->book, p.q))) return MELSPEC_OK;
    st->cache.key.invalidate();
    const char *err = nullptr;
    return plan_status(stream_plan_push(st->geom, st->book, p.q.ids, p.q.lens, p.q.n, p.flush, st->cache.pl, &err), err);
}

// the push is through: the book moves on
void stream_commit(melspec_stream *st, const StreamPush &p, uint32_t *h_frames) {
    const uint32_t *frames = st->cache.pl.frames.data();
    stream_commit_push(st->geom, st->book, p.q.ids, p.q.lens, p.q.n, p.flush);
    for (uint32_t i = 0; st->vad_on && i < p.q.n; ++i) st->vad_count[p.q.ids[i]] += frames[i];
    if (h_frames) std::memcpy(h_frames, frames, static_cast<size_t>(p.q.n) * sizeof(uint32_t));
}

// the bank's frame stage behind core_run's scatter: spectra, or mel rows (planned, or the cached plan again) and the detector
int stream_frames(melspec_stream *st, const StreamPush &p, const StreamEntry *d_e, hipStream_t s) {
    melspec_ctx *c = st->ctx;
    const StreamPlan &pl = st->cache.pl;
    const PushQuery &q = p.q;
    const uint32_t n = q.n;
    float *state = static_cast<float *>(st->core.state.p);
    if (p.emit.stft) {
        std::vector<uint64_t> oo(n);            // complex elements, entries back to back
        uint64_t cur = 0;
        const uint64_t bins = melspec_stft_bins(c, p.emit.full);
        for (uint32_t i = 0; i < n; ++i) { oo[i] = cur; cur += pl.frames[i] * bins; }
        return melspec_stft_ragged_device(c, state, pl.off.data(), pl.len.data(), n, const_cast<void *>(q.d_out), q.h_out_off ? q.h_out_off : oo.data(),
                                          p.emit.dtype, p.emit.full, s);
    }
    const int out_only_io = q.io & ~15;       // the frame kernel's PCM is the f32 state whatever the chunks were
    int rc;
    if (p.hit) {
        rc = launch_ctx(c, st->cache.plan.desc, s, out_only_io);
    } else {
        // melspec_compute_ragged_device with the plan kept: frames per entry are the plan's, the ring is the bank's own
        std::vector<uint64_t> fr(pl.frames.begin(), pl.frames.end());
        RaggedSlot *pslot = nullptr;
        rc = plan_ragged(st->core.plan_ring, s, state, static_cast<float *>(const_cast<void *>(q.d_out)), pl.off.data(), fr,
                         q.h_out_off ? q.h_out_off : pl.out_off.data(), n, c->n_mels, q.fpu, st->cache.plan, pslot);
        if (!rc) rc = launch_ctx(c, st->cache.plan.desc, s, out_only_io);
        plan_ragged_done(pslot, s);
        if (!rc && st->cache.key.fill(st->geom, st->book, q)) st->cache.d_e = d_e;
    }
    if (rc || !st->vad_on) return rc;
    StreamVadParams vp{};
    vp.entries = d_e; vp.rows = static_cast<const float *>(q.d_out);
    vp.state = static_cast<StreamVadState *>(st->vad_state.p); vp.prev = static_cast<float *>(st->vad_prev.p);
    vp.acts = reinterpret_cast<VadActivity *>(p.d_acts);
    vp.n_mels = st->geom.n_mels; vp.min_mel = st->vad.min_mel; vp.min_y = st->vad.min_y; vp.min_x = st->vad.min_x;
    vp.thr = st->vad.min_energy * st->vad.min_energy;
    uint32_t most = 0;
    for (uint32_t i = 0; i < n; ++i) most = std::max(most, pl.frames[i]);
    hipLaunchKernelGGL(stream_vad_kernel, dim3(n), dim3(most <= 1 ? 64 : most <= 2 ? 128 : 256), 0, s, vp);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

// scatter (optional) -> frames -> carry update, all on one stream.  d_src: the chunks (NULL: in the slots already)
int stream_run(melspec_stream *st, StreamPush &p, const void *d_src, hipStream_t s) {
    const StreamPlan &pl = st->cache.pl;
    if (st->vad_on && p.emit.stft) return fail(MELSPEC_ERR_UNSUPPORTED, "the detector stage is on: it needs the mel rows of every push");
    if (st->vad_on && pl.total_frames && !p.d_acts) {                                           // records nobody asked for: internal buffer
        HIP_TRY(hipSetDevice(st->core.device));
        if (int rc = st->vad_acts.ensure(pl.total_frames * sizeof(melspec_vad_activity))) return rc;
        p.d_acts = static_cast<melspec_vad_activity *>(st->vad_acts.p);
    }
    bool zero_fill = false;
    for (uint32_t i = 0; p.flush && i < p.q.n && !zero_fill; ++i) zero_fill = pl.entries[i].zero_fill != 0;
    const PushArgs a{d_src, p.q.io & 15, p.q.h_src_off, const_cast<void *>(p.q.d_out), p.q.h_out_off, s, zero_fill};
    return core_run(st->core, pl.entries.data(), p.q.n, pl.total_frames, a, p.hit ? st->cache.d_e : nullptr, nullptr, 0,
                    [&](const StreamEntry *d_e, const void *) { return stream_frames(st, p, d_e, s); });
}
}  // namespace

extern "C" {

int melspec_stream_create(melspec_stream **out, melspec_ctx *ctx, uint32_t n_streams, uint32_t max_chunk) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx) return fail(MELSPEC_ERR_INVALID_ARG, "ctx is NULL");
    if (n_streams == 0 || max_chunk == 0) return fail(MELSPEC_ERR_INVALID_ARG, "n_streams and max_chunk must be > 0");
    if (ctx->hop_size > ctx->fft_size) return fail(MELSPEC_ERR_UNSUPPORTED, "streaming needs hop_size <= fft_size");
    melspec_stream *st = new (std::nothrow) melspec_stream();
    if (!st) return fail(MELSPEC_ERR_INTERNAL, "out of host memory");
    st->ctx = ctx;
    st->geom = stream_geometry(static_cast<uint32_t>(ctx->fft_size), static_cast<uint32_t>(ctx->hop_size), static_cast<uint32_t>(ctx->n_mels),
                               n_streams, max_chunk);
    st->book.reset(n_streams);
    if (int rc = core_create(st->core, ctx->dev.device, ctx->stream, n_streams, st->geom.stride, st->geom.in_off)) { melspec_stream_destroy(st); return rc; }
    *out = st;
    return MELSPEC_OK;
}

void melspec_stream_destroy(melspec_stream *st) {
    if (!st) return;
    core_destroy(st->core);
    st->vad_state.release(); st->vad_prev.release(); st->vad_acts.release();
    delete st;
}

int melspec_stream_reset(melspec_stream *st, const uint32_t *ids, uint32_t n) {
    if (!st) return fail(MELSPEC_ERR_INVALID_ARG, "stream bank is NULL");
    if (int rc = core_reset_slots(st->core, ids, n)) return rc;      // a bad id: nothing has been touched
    st->cache.key.invalidate();
    hipStream_t s = st->core.stream;
    if (!ids) {
        st->book.reset(st->geom.n_streams);
        if (st->vad_on) {
            HIP_TRY(hipMemsetAsync(st->vad_state.p, 0, static_cast<size_t>(st->geom.n_streams) * sizeof(StreamVadState), s));
            std::fill(st->vad_count.begin(), st->vad_count.end(), 0ull);
        }
    }
    for (uint32_t i = 0; ids && i < n; ++i) {
        st->book.pending[ids[i]] = 0; st->book.idx[ids[i]] = 0;
        if (st->vad_on) {
            HIP_TRY(hipMemsetAsync(static_cast<StreamVadState *>(st->vad_state.p) + ids[i], 0, sizeof(StreamVadState), s));
            st->vad_count[ids[i]] = 0;
        }
    }
    HIP_TRY(hipStreamSynchronize(s));
    return MELSPEC_OK;
}

size_t melspec_stream_frames_after(const melspec_stream *st, uint32_t id, uint32_t n_new) {
    if (!st || id >= st->geom.n_streams) return 0;
    return stream_frames_after(st->geom, st->book, id, n_new);
}

float *melspec_stream_input_ptr(melspec_stream *st, uint32_t id) { return st ? core_input_ptr(st->core, id) : nullptr; }

static_assert(sizeof(melspec_vad_activity) == 8 && sizeof(VadActivity) == 8, "the activity record is 8 bytes on both sides of the ABI");
// io / d_chunks / h_src_offsets: melspec_stream_push_device_io -- the element types, and chunks that lie in the caller's own device
// buffer (NULL: already in the slots, at melspec_stream_input_ptr)
static int stream_push_device_impl(melspec_stream *st, const uint32_t *ids, const uint32_t *lens, uint32_t n, void *d_out,
                                   const uint64_t *h_out_offsets, uint32_t *h_frames, melspec_vad_activity *d_acts, bool want_acts,
                                   void *stream, int io = 0, const void *d_chunks = nullptr, const uint64_t *h_src_offsets = nullptr) {
    if (!st) return fail(MELSPEC_ERR_INVALID_ARG, "stream bank is NULL");
    if (want_acts && !st->vad_on) return fail(MELSPEC_ERR_INVALID_ARG, "the detector stage is off (melspec_stream_enable_vad)");
    if (n == 0) return MELSPEC_OK;
    if (!ids || !lens) return fail(MELSPEC_ERR_INVALID_ARG, "ids/lens is NULL");
    StreamPush p;
    p.q.io = io; p.q.d_out = d_out; p.q.h_out_off = h_out_offsets; p.q.h_src_off = d_chunks ? h_src_offsets : nullptr;
    p.d_acts = d_acts;
    int rc = stream_prepare(st, p, ids, lens, n);
    if (rc) return rc;
    if (want_acts && st->cache.pl.total_frames && !d_acts) return fail(MELSPEC_ERR_INVALID_ARG, "d_acts is NULL");
    if ((rc = stream_run(st, p, d_chunks, stream ? static_cast<hipStream_t>(stream) : st->core.stream))) return rc;
    stream_commit(st, p, h_frames);
    return MELSPEC_OK;
}

int melspec_stream_push_device(melspec_stream *st, const uint32_t *ids, const uint32_t *lens, uint32_t n, float *d_out,
                               const uint64_t *h_out_offsets, uint32_t *h_frames, void *stream) {
    return stream_push_device_impl(st, ids, lens, n, d_out, h_out_offsets, h_frames, nullptr, false, stream);
}

int melspec_stream_push_device_vad(melspec_stream *st, const uint32_t *ids, const uint32_t *lens, uint32_t n, float *d_out,
                                   const uint64_t *h_out_offsets, uint32_t *h_frames, melspec_vad_activity *d_acts, void *stream) {
    return stream_push_device_impl(st, ids, lens, n, d_out, h_out_offsets, h_frames, d_acts, true, stream);
}

int melspec_stream_enable_vad(melspec_stream *st, const melspec_vad_settings *settings) {
    if (!st) return fail(MELSPEC_ERR_INVALID_ARG, "stream bank is NULL");
    HIP_TRY(hipSetDevice(st->core.device));
    HIP_TRY(hipStreamSynchronize(st->core.stream));
    if (!settings) { st->vad_on = false; return MELSPEC_OK; }
    if (settings->min_x > kStreamVadMaxX) return fail(MELSPEC_ERR_UNSUPPORTED, "min_x above 66: the column history of a stream is 64 bits");
    if (settings->min_x < 0 || settings->min_y < 0 || settings->min_mel < 0) return fail(MELSPEC_ERR_INVALID_ARG, "negative detection setting");
    const size_t ns = st->geom.n_streams;
    int rc = st->vad_state.ensure(ns * sizeof(StreamVadState));
    if (rc) return rc;
    if ((rc = st->vad_prev.ensure(ns * 2 * st->geom.n_mels * sizeof(float) + 16))) return rc;
    HIP_TRY(hipMemset(st->vad_state.p, 0, ns * sizeof(StreamVadState)));
    HIP_TRY(hipMemset(st->vad_prev.p, 0, ns * 2 * st->geom.n_mels * sizeof(float)));
    st->vad_count.assign(ns, 0ull);
    st->vad = *settings;
    st->vad_on = true;
    return MELSPEC_OK;
}

uint64_t melspec_stream_vad_frames(const melspec_stream *st, uint32_t id) {
    if (!st || !st->vad_on || id >= st->geom.n_streams) return 0;
    return st->vad_count[id];
}

// p: what the push is besides its chunks -- a flush, spectra, typed ends (p.q.io, melspec_stream_push_host_io / _flush_host_io: samples
// holds elements of the sample type, out receives elements of the row type), the caller's activity buffer
static int stream_push_host_impl(melspec_stream *st, const uint32_t *ids, const void *samples, const uint32_t *lens, uint32_t n,
                                 void *out, size_t out_capacity, uint32_t *h_frames, StreamPush p = StreamPush()) {
    if (!st) return fail(MELSPEC_ERR_INVALID_ARG, "stream bank is NULL");
    if (p.want_acts && !st->vad_on) return fail(MELSPEC_ERR_INVALID_ARG, "the detector stage is off (melspec_stream_enable_vad)");
    if (n == 0) return MELSPEC_OK;
    if (!ids || (!p.flush && !lens)) return fail(MELSPEC_ERR_INVALID_ARG, "ids/lens is NULL");
    p.q.d_out = st->core.out.p;
    int rc = stream_prepare(st, p, ids, lens, n);
    if (rc) return rc;
    const StreamPlan &pl = st->cache.pl;
    if (p.want_acts && pl.total_frames > p.acts_capacity) return fail(MELSPEC_ERR_CAPACITY, "activity buffer too small");
    if (p.want_acts && pl.total_frames && !p.acts) return fail(MELSPEC_ERR_INVALID_ARG, "acts is NULL");
    const StreamEmit &e = p.emit;
    // elements the caller receives: floats (mel rows) or complex values (spectra)
    const uint64_t need = pl.total_frames * (e.stft ? melspec_stft_bins(st->ctx, e.full) : static_cast<uint64_t>(st->ctx->n_mels));
    const size_t esz = e.stft ? (e.dtype == MELSPEC_STFT_F64 ? 16 : 8) : io_out_bytes(p.q.io >> 4);
    const HostPush h{samples, out, out_capacity, need, io_pcm_bytes(p.q.io & 15), esz};
    rc = core_push_host(st->core, pl.entries.data(), n, h, [&](const void *d_src, void *d_out, hipStream_t s) {
        p.q.d_out = d_out;
        if (int rc2 = stream_run(st, p, d_src, s)) return rc2;      // the records go to the bank's own buffer (p.d_acts is NULL)
        if (p.want_acts && pl.total_frames) HIP_TRY(hipMemcpyAsync(p.acts, p.d_acts, pl.total_frames * sizeof(melspec_vad_activity), hipMemcpyDeviceToHost, s));
        return static_cast<int>(MELSPEC_OK);
    });
    if (rc) return rc;
    stream_commit(st, p, h_frames);
    return MELSPEC_OK;
}

int melspec_stream_push_host(melspec_stream *st, const uint32_t *ids, const float *samples, const uint32_t *lens, uint32_t n,
                             float *out, size_t out_capacity_floats, uint32_t *h_frames) {
    return stream_push_host_impl(st, ids, samples, lens, n, out, out_capacity_floats, h_frames);
}

int melspec_stream_push_host_stft(melspec_stream *st, const uint32_t *ids, const float *samples, const uint32_t *lens, uint32_t n,
                                  void *out, size_t out_capacity_complex, uint32_t *h_frames, int dtype, int full) {
    if (st) { const int rc = stft_args(st->ctx, dtype); if (rc) return rc; }
    StreamPush p;
    p.emit.stft = true; p.emit.dtype = dtype; p.emit.full = full;
    return stream_push_host_impl(st, ids, samples, lens, n, out, out_capacity_complex, h_frames, p);
}

int melspec_stream_flush_host(melspec_stream *st, const uint32_t *ids, uint32_t n, float *out, size_t out_capacity_floats,
                              uint32_t *h_frames) {
    StreamPush p;
    p.flush = true;
    return stream_push_host_impl(st, ids, nullptr, nullptr, n, out, out_capacity_floats, h_frames, p);
}

int melspec_stream_push_host_vad(melspec_stream *st, const uint32_t *ids, const float *samples, const uint32_t *lens, uint32_t n,
                                 float *out, size_t out_capacity_floats, uint32_t *h_frames, melspec_vad_activity *acts, size_t acts_capacity) {
    StreamPush p;
    p.want_acts = true; p.acts = acts; p.acts_capacity = acts_capacity;
    return stream_push_host_impl(st, ids, samples, lens, n, out, out_capacity_floats, h_frames, p);
}

int melspec_stream_flush_host_vad(melspec_stream *st, const uint32_t *ids, uint32_t n, float *out, size_t out_capacity_floats,
                                  uint32_t *h_frames, melspec_vad_activity *acts, size_t acts_capacity) {
    StreamPush p;
    p.flush = p.want_acts = true; p.acts = acts; p.acts_capacity = acts_capacity;
    return stream_push_host_impl(st, ids, nullptr, nullptr, n, out, out_capacity_floats, h_frames, p);
}

// ---- int16 PCM chunks in / f16, bf16 rows out -------------------------------------------------------------------------------------
// The state stays f32: int16 samples are converted where the chunk is scattered into it (stream_scatter_kernel<io_s16>), so every
// geometry takes them; 16-bit rows are the six-frame n_fft = 400 kernels' typed stores (launch_ctx with the out half of the code).
// 0: go on (io = pcm_dtype | out_dtype << 4); otherwise the status to return.  Nothing is queued and the bank is untouched on a refusal.
static int stream_io_args(const melspec_stream *st, int pcm_dtype, int out_dtype, int &io) {
    if (!st) return fail(MELSPEC_ERR_INVALID_ARG, "stream bank is NULL");
    if (int rc = io_dtypes(pcm_dtype, out_dtype, io)) return rc;
    if (out_dtype == MELSPEC_OUT_F32) return MELSPEC_OK;
    const melspec_ctx *c = st->ctx;
    if (!ctx_supports_io(c)) {
        g_last_error = "f16, bf16 rows are computed by the n_fft = 400 contexts with Whisper's 80- or 128-mel bank only; this bank's context is n_fft = " +
                       std::to_string(c->fft_size) + ", hop = " + std::to_string(c->hop_size) + ", n_mels = " + std::to_string(c->n_mels) +
                       (c->fast ? " (another filterbank)" : "");
        return MELSPEC_ERR_UNSUPPORTED;
    }
    if (st->vad_on) return fail(MELSPEC_ERR_UNSUPPORTED, "the detector stage is on: it reads f32 rows (out_dtype must be MELSPEC_OUT_F32)");
    return MELSPEC_OK;
}

int melspec_stream_supports_io(const melspec_stream *st, int pcm_dtype, int out_dtype) {
    if (!st || !io_pcm_known(pcm_dtype) || !io_out_known(out_dtype)) return 0;
    return out_dtype == MELSPEC_OUT_F32 || ctx_supports_io(st->ctx) ? 1 : 0;
}

int melspec_stream_push_host_io(melspec_stream *st, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n,
                                void *out, int out_dtype, size_t out_capacity_elems, uint32_t *h_frames) {
    int io, rc = stream_io_args(st, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    StreamPush p;
    p.q.io = io;
    return stream_push_host_impl(st, ids, samples, lens, n, out, out_capacity_elems, h_frames, p);
}

int melspec_stream_flush_host_io(melspec_stream *st, const uint32_t *ids, uint32_t n, void *out, int out_dtype, size_t out_capacity_elems,
                                 uint32_t *h_frames) {
    int io, rc = stream_io_args(st, MELSPEC_PCM_F32, out_dtype, io);
    if (rc) return rc;
    StreamPush p;
    p.flush = true; p.q.io = io;
    return stream_push_host_impl(st, ids, nullptr, nullptr, n, out, out_capacity_elems, h_frames, p);
}

int melspec_stream_push_device_io(melspec_stream *st, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets,
                                  const uint32_t *lens, uint32_t n, void *d_out, int out_dtype, const uint64_t *h_out_offsets,
                                  uint32_t *h_frames, void *stream) {
    int io, rc = stream_io_args(st, pcm_dtype, out_dtype, io);
    if (rc) return rc;
    if (!d_chunks && pcm_dtype != MELSPEC_PCM_F32)
        return fail(MELSPEC_ERR_INVALID_ARG, "d_chunks is NULL: the chunks are at melspec_stream_input_ptr, which holds f32 (pcm_dtype must be MELSPEC_PCM_F32)");
    if (!io && !d_chunks) return melspec_stream_push_device(st, ids, lens, n, static_cast<float *>(d_out), h_out_offsets, h_frames, stream);
    if (io_misaligned(d_chunks, d_out, io))
        return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type");
    return stream_push_device_impl(st, ids, lens, n, d_out, h_out_offsets, h_frames, nullptr, false, stream, io, d_chunks, h_src_offsets);
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// 8-bit quantisation + TGA container (src/quant.rs)
// ------------------------------------------------------------------------------------
struct melspec_tga {
    DeviceInfo dev;
    hipStream_t stream = nullptr;
    DevBuf keys, ranges, h2d, d2h, unit_ext;       // unit_ext: the mel kernel's per-unit extremes (melspec_tga_encode_pcm_uniform_device)
    // the min/max keys are one scratch buffer per handle, used in stream order: a call on another stream first waits for
    // the stream that used it last
    hipStream_t keys_stream = nullptr;
    bool keys_used = false;
};

namespace {
size_t round_up4(size_t v) { return (v + 3) & ~static_cast<size_t>(3); }

struct TgaLayout { uint32_t chunks; uint32_t chunk_w; size_t chunk_stride; size_t last_bytes; };
TgaLayout tga_layout(uint32_t rows, uint64_t width) {
    TgaLayout l{};
    if (width == 0) return l;
    l.chunks = static_cast<uint32_t>((width + kTgaMaxWidth - 1) / kTgaMaxWidth);
    l.chunk_w = static_cast<uint32_t>(width < kTgaMaxWidth ? width : kTgaMaxWidth);
    l.chunk_stride = round_up4(kTgaHeader + static_cast<size_t>(rows) * l.chunk_w);
    l.last_bytes = kTgaHeader + static_cast<size_t>(rows) * (width - static_cast<uint64_t>(l.chunks - 1) * l.chunk_w);
    return l;
}

// fills the descriptor and the launch shape shared by encode and decode
int quant_plan(melspec_tga *q, QuantDesc &d, const void *img, size_t image_stride, uint32_t rows, uint64_t width, uint32_t n_images,
               const void *blob, size_t blob_stride, bool header, uint32_t &items, uint32_t &bpi_px, uint32_t &bpi_dw) {
    if (width > 0xffffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "image wider than 2^32-1 columns");
    d = QuantDesc{};
    d.rows = rows; d.width = static_cast<uint32_t>(width); d.n_images = n_images;
    d.img_stride = image_stride; d.blob_stride = blob_stride;
    d.header = header ? kTgaHeader : 0;
    if (header) {
        const TgaLayout l = tga_layout(rows, width);
        d.chunks = l.chunks; d.chunk_w = l.chunk_w; d.chunk_stride = l.chunk_stride;
        if (blob_stride % 4 || blob_stride < l.chunk_stride * l.chunks)
            return fail(MELSPEC_ERR_INVALID_ARG, "blob_stride must be a multiple of 4 and >= n_chunks * chunk_stride (melspec_tga_layout)");
    } else {
        d.chunks = 1; d.chunk_w = d.width; d.chunk_stride = 0;
        if (blob_stride % 4) return fail(MELSPEC_ERR_INVALID_ARG, "blob_stride must be a multiple of 4");
    }
    if (reinterpret_cast<uintptr_t>(blob) % 4) return fail(MELSPEC_ERR_INVALID_ARG, "blob pointer must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(img) % 4) return fail(MELSPEC_ERR_INVALID_ARG, "image pointer must be 4-byte aligned");
    d.vec = d.chunks == 1 && reinterpret_cast<uintptr_t>(img) % 16 == 0 && (n_images == 1 || image_stride % 4 == 0);
    const uint64_t items64 = static_cast<uint64_t>(n_images) * d.chunks;
    const uint64_t npx = static_cast<uint64_t>(rows) * d.chunk_w;
    const uint64_t bpx = (npx + kQuantPxPerBlock - 1) / kQuantPxPerBlock;
    const uint64_t bdw = ((d.header + npx + 3) / 4 + kQuantDwPerBlock - 1) / kQuantDwPerBlock;
    if (items64 * bpx > 0x7fffffffull || items64 * bdw > 0x7fffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "batch too large for one launch");
    items = static_cast<uint32_t>(items64); bpi_px = static_cast<uint32_t>(bpx); bpi_dw = static_cast<uint32_t>(bdw);
    int rc = q->keys.ensure(items64 * 2 * sizeof(uint32_t) + 16);
    if (rc) return rc;
    d.keys = static_cast<uint32_t *>(q->keys.p);
    return MELSPEC_OK;
}

int quant_encode(melspec_tga *q, const float *d_img, size_t image_stride, uint32_t rows, uint64_t width, uint32_t n_images,
                 uint8_t *d_blob, size_t blob_stride, bool header, float *d_ranges, hipStream_t stream) {
    if (n_images == 0 || width == 0 || rows == 0) return MELSPEC_OK;
    if (!d_img || !d_blob) return fail(MELSPEC_ERR_INVALID_ARG, "image/blob pointer is NULL");
    HIP_TRY(hipSetDevice(q->dev.device));
    QuantDesc d;
    uint32_t items, bpx, bdw;
    int rc = quant_plan(q, d, d_img, image_stride, rows, width, n_images, d_blob, blob_stride, header, items, bpx, bdw);
    if (rc) return rc;
    d.img = d_img; d.blob = d_blob; d.ranges = d_ranges;
    if (q->keys_used && q->keys_stream != stream) HIP_TRY(hipStreamSynchronize(q->keys_stream));
    q->keys_used = true; q->keys_stream = stream;
    hipLaunchKernelGGL(quant_init_keys_kernel, dim3((items + 255) / 256), dim3(256), 0, stream, d.keys, items);
    hipLaunchKernelGGL(quant_minmax_kernel, dim3(items * bpx), dim3(kQuantThreads), 0, stream, d, bpx);
    hipLaunchKernelGGL(quant_encode_kernel, dim3(items * bdw), dim3(kQuantThreads), 0, stream, d, bdw);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int quant_decode(melspec_tga *q, const uint8_t *d_blob, size_t blob_stride, uint32_t rows, uint64_t width, uint32_t n_images,
                 float *d_img, size_t image_stride, bool header, const float *d_ranges, hipStream_t stream) {
    if (n_images == 0 || width == 0 || rows == 0) return MELSPEC_OK;
    if (!d_img || !d_blob) return fail(MELSPEC_ERR_INVALID_ARG, "image/blob pointer is NULL");
    if (!header && !d_ranges) return fail(MELSPEC_ERR_INVALID_ARG, "range pointer is NULL");
    HIP_TRY(hipSetDevice(q->dev.device));
    QuantDesc d;
    uint32_t items, bpx, bdw;
    int rc = quant_plan(q, d, d_img, image_stride, rows, width, n_images, d_blob, blob_stride, header, items, bpx, bdw);
    if (rc) return rc;
    d.img_out = d_img; d.blob = const_cast<uint8_t *>(d_blob); d.ranges = const_cast<float *>(d_ranges);
    hipLaunchKernelGGL(quant_decode_kernel, dim3(items * bdw), dim3(kQuantThreads), 0, stream, d, bdw);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}
}  // namespace

extern "C" {

int melspec_tga_create(melspec_tga **out, int device) {
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    *out = nullptr;
    DeviceInfo info;
    int rc = pick_device(device, info);
    if (rc) return rc;
    melspec_tga *q = new (std::nothrow) melspec_tga();
    if (!q) return fail(MELSPEC_ERR_INTERNAL, "out of host memory");
    q->dev = info;
    if (hipSetDevice(info.device) != hipSuccess || hipStreamCreate(&q->stream) != hipSuccess) {
        delete q;
        return fail(MELSPEC_ERR_UNAVAILABLE, "hipStreamCreate failed");
    }
    *out = q;
    return MELSPEC_OK;
}

void melspec_tga_destroy(melspec_tga *q) {
    if (!q) return;
    if (q->dev.device >= 0) (void)hipSetDevice(q->dev.device);
    if (q->stream) { (void)hipStreamSynchronize(q->stream); (void)hipStreamDestroy(q->stream); }
    q->keys.release(); q->ranges.release(); q->h2d.release(); q->d2h.release(); q->unit_ext.release();
    delete q;
}

int melspec_tga_layout(int n_mels, size_t width, uint32_t *n_chunks, size_t *chunk_stride, size_t *last_chunk_bytes) {
    if (n_mels <= 0 || n_mels > 65535) return fail(MELSPEC_ERR_INVALID_ARG, "n_mels must be in 1..65535");
    const TgaLayout l = tga_layout(static_cast<uint32_t>(n_mels), width);
    if (n_chunks) *n_chunks = l.chunks;
    if (chunk_stride) *chunk_stride = l.chunk_stride;
    if (last_chunk_bytes) *last_chunk_bytes = l.last_bytes;
    return MELSPEC_OK;
}

int melspec_tga_encode_device(melspec_tga *q, const float *d_images, size_t image_stride, int n_mels, size_t width,
                              uint32_t n_images, uint8_t *d_blobs, size_t blob_stride, void *stream) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (n_mels <= 0 || n_mels > 65535) return fail(MELSPEC_ERR_INVALID_ARG, "n_mels must be in 1..65535");
    if (image_stride < static_cast<size_t>(n_mels) * width) return fail(MELSPEC_ERR_INVALID_ARG, "image_stride < n_mels * width");
    return quant_encode(q, d_images, image_stride, static_cast<uint32_t>(n_mels), width, n_images, d_blobs, blob_stride, true, nullptr,
                        stream ? static_cast<hipStream_t>(stream) : q->stream);
}

// PCM -> TGA bytes with the image read once: while it stores the image (mel-major) the mel kernel leaves the extremes of every work
// unit behind (BatchDesc::d_unit_ext: one wave-wide reduction and one 8-byte store per unit), a one-wave-per-image kernel folds them
// into the quantiser's keys, so only the encoding pass reads the image again -- 5 B/pixel moved for 5 B/pixel algorithmic, where minmax + encode moved 9 ("4x smaller D2H").  The bytes are
// those of melspec_compute_uniform_device_interleaved(.., major_column_order = 0, min_width) followed by melspec_tga_encode_device.
int melspec_tga_encode_pcm_uniform_device(melspec_tga *q, melspec_ctx *c, const float *d_pcm, uint64_t clip_stride, uint64_t clip_len,
                                          uint32_t n_clips, uint64_t min_width, float *d_images, uint8_t *d_blobs, size_t blob_stride,
                                          void *stream) {
    if (!q || !c) return fail(MELSPEC_ERR_INVALID_ARG, "tga / ctx is NULL");
    if (q->dev.device != c->dev.device) return fail(MELSPEC_ERR_INVALID_ARG, "the codec and the context are on different devices");
    if (min_width % 2 != 0) return fail(MELSPEC_ERR_INVALID_ARG, "min_width must be even");   // src/mel.rs:488
    if (n_clips == 0) return MELSPEC_OK;
    uint64_t fpc; ctx_num_frames(c, clip_len, fpc);
    if (fpc == 0) return fail(MELSPEC_ERR_INVALID_ARG, "frames is empty");                      // src/mel.rs:487
    if (!d_pcm || !d_images || !d_blobs) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is NULL");
    HIP_TRY(hipSetDevice(c->dev.device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
    const uint64_t width = interleaved_width(fpc, min_width);
    const size_t image_stride = static_cast<size_t>(c->n_mels) * width;
    if (!c->fast || width > kTgaMaxWidth) {
        // geometries on the generic / 512-point kernels, and images wider than one TGA chunk: the two-pass form
        int rc = melspec_compute_uniform_device_interleaved(c, d_pcm, clip_stride, clip_len, n_clips, d_images, 0, min_width, s);
        if (rc) return rc;
        return melspec_tga_encode_device(q, d_images, image_stride, c->n_mels, width, n_clips, d_blobs, blob_stride, s);
    }
    QuantDesc d;
    uint32_t items, bpx, bdw;
    int rc = quant_plan(q, d, d_images, image_stride, static_cast<uint32_t>(c->n_mels), width, n_clips, d_blobs, blob_stride, true, items, bpx, bdw);
    if (rc) return rc;
    d.img = d_images; d.blob = d_blobs; d.ranges = nullptr;
    if (q->keys_used && q->keys_stream != s) HIP_TRY(hipStreamSynchronize(q->keys_stream));
    q->keys_used = true; q->keys_stream = s;
    BatchPlan pl = plan_uniform(d_pcm, d_images, clip_stride, fpc, n_clips, c->n_mels, ctx_frames_per_unit(c, true), width, true);
    if ((rc = q->unit_ext.ensure(static_cast<size_t>(pl.desc.n_units) * 2 * sizeof(int) + 16))) return rc;
    pl.desc.d_unit_ext = static_cast<int *>(q->unit_ext.p);
    if ((rc = launch_ctx(c, pl.desc, s))) return rc;
    // one chunk per image: item == clip; its units' records -> its keys
    hipLaunchKernelGGL(quant_keys_from_units_kernel, dim3(n_clips), dim3(64), 0, s, pl.desc.d_unit_ext, pl.desc.units_per_clip, n_clips, d.keys);
    hipLaunchKernelGGL(quant_encode_kernel, dim3(items * bdw), dim3(kQuantThreads), 0, s, d, bdw);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_tga_decode_device(melspec_tga *q, const uint8_t *d_blobs, size_t blob_stride, int n_mels, size_t width,
                              uint32_t n_images, float *d_images, size_t image_stride, void *stream) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (n_mels <= 0 || n_mels > 65535) return fail(MELSPEC_ERR_INVALID_ARG, "n_mels must be in 1..65535");
    if (image_stride < static_cast<size_t>(n_mels) * width) return fail(MELSPEC_ERR_INVALID_ARG, "image_stride < n_mels * width");
    return quant_decode(q, d_blobs, blob_stride, static_cast<uint32_t>(n_mels), width, n_images, d_images, image_stride, true, nullptr,
                        stream ? static_cast<hipStream_t>(stream) : q->stream);
}

int melspec_quantize_device(melspec_tga *q, const float *d_frame, size_t n, uint8_t *d_out, float *d_range, void *stream) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (!d_range) return fail(MELSPEC_ERR_INVALID_ARG, "range pointer is NULL");
    return quant_encode(q, d_frame, n, 1, n, 1, d_out, round_up4(n), false, d_range, stream ? static_cast<hipStream_t>(stream) : q->stream);
}

int melspec_dequantize_device(melspec_tga *q, const uint8_t *d_data, size_t n, const float *d_range, float *d_out, void *stream) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    return quant_decode(q, d_data, round_up4(n), 1, n, 1, d_out, n, false, d_range, stream ? static_cast<hipStream_t>(stream) : q->stream);
}

int melspec_tga_synchronize(melspec_tga *q) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    HIP_TRY(hipStreamSynchronize(q->stream));
    return MELSPEC_OK;
}

int melspec_quantize_host(melspec_tga *q, const float *frame, size_t n, uint8_t *out, float *range) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (!range) return fail(MELSPEC_ERR_INVALID_ARG, "range pointer is NULL");
    if (n == 0) { range[0] = INFINITY; range[1] = -INFINITY; return MELSPEC_OK; }       // the folds' start values
    if (!frame || !out) return fail(MELSPEC_ERR_INVALID_ARG, "frame/out is NULL");
    HIP_TRY(hipSetDevice(q->dev.device));
    int rc;
    if ((rc = q->h2d.ensure(n * sizeof(float)))) return rc;
    if ((rc = q->d2h.ensure(round_up4(n) + 16))) return rc;
    if ((rc = q->ranges.ensure(16))) return rc;
    HIP_TRY(hipMemcpyAsync(q->h2d.p, frame, n * sizeof(float), hipMemcpyHostToDevice, q->stream));
    if ((rc = melspec_quantize_device(q, static_cast<const float *>(q->h2d.p), n, static_cast<uint8_t *>(q->d2h.p),
                                      static_cast<float *>(q->ranges.p), q->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, q->d2h.p, n, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipMemcpyAsync(range, q->ranges.p, 2 * sizeof(float), hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    return MELSPEC_OK;
}

int melspec_dequantize_host(melspec_tga *q, const uint8_t *data, size_t n, const float *range, float *out) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (n == 0) return MELSPEC_OK;
    if (!data || !range || !out) return fail(MELSPEC_ERR_INVALID_ARG, "data/range/out is NULL");
    HIP_TRY(hipSetDevice(q->dev.device));
    int rc;
    if ((rc = q->h2d.ensure(round_up4(n) + 16))) return rc;
    if ((rc = q->d2h.ensure(n * sizeof(float)))) return rc;
    if ((rc = q->ranges.ensure(16))) return rc;
    HIP_TRY(hipMemcpyAsync(q->h2d.p, data, n, hipMemcpyHostToDevice, q->stream));
    HIP_TRY(hipMemcpyAsync(q->ranges.p, range, 2 * sizeof(float), hipMemcpyHostToDevice, q->stream));
    if ((rc = melspec_dequantize_device(q, static_cast<const uint8_t *>(q->h2d.p), n, static_cast<const float *>(q->ranges.p),
                                        static_cast<float *>(q->d2h.p), q->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, q->d2h.p, n * sizeof(float), hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    return MELSPEC_OK;
}

int melspec_tga_encode_host(melspec_tga *q, const float *data, size_t len, int n_mels, uint8_t *out, size_t out_capacity,
                            uint32_t *n_chunks) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (n_chunks) *n_chunks = 0;
    if (n_mels <= 0 || n_mels > 65535) return fail(MELSPEC_ERR_INVALID_ARG, "n_mels must be in 1..65535");
    if (len % static_cast<size_t>(n_mels)) return fail(MELSPEC_ERR_INVALID_ARG, "data length is not a multiple of n_mels");
    const size_t width = len / n_mels;
    if (width == 0) return MELSPEC_OK;
    if (!data || !out) return fail(MELSPEC_ERR_INVALID_ARG, "data/out is NULL");
    const TgaLayout l = tga_layout(static_cast<uint32_t>(n_mels), width);
    const size_t region = l.chunk_stride * l.chunks;
    if (out_capacity < region - l.chunk_stride + l.last_bytes) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
    HIP_TRY(hipSetDevice(q->dev.device));
    int rc;
    if ((rc = q->h2d.ensure(len * sizeof(float)))) return rc;
    if ((rc = q->d2h.ensure(region))) return rc;
    HIP_TRY(hipMemcpyAsync(q->h2d.p, data, len * sizeof(float), hipMemcpyHostToDevice, q->stream));
    if ((rc = melspec_tga_encode_device(q, static_cast<const float *>(q->h2d.p), len, n_mels, width, 1,
                                        static_cast<uint8_t *>(q->d2h.p), region, q->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(out, q->d2h.p, region - l.chunk_stride + l.last_bytes, hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    if (n_chunks) *n_chunks = l.chunks;
    return MELSPEC_OK;
}

int melspec_tga_decode_host(melspec_tga *q, const uint8_t *blob, size_t n_bytes, float *out, size_t out_capacity, size_t *n_values) {
    if (!q) return fail(MELSPEC_ERR_INVALID_ARG, "tga is NULL");
    if (n_values) *n_values = 0;
    if (!blob || n_bytes < kTgaHeader) return fail(MELSPEC_ERR_INVALID_ARG, "failed to fill whole buffer");   // read_exact, src/quant.rs:74-75
    const size_t npx = n_bytes - kTgaHeader;
    if (npx == 0) return MELSPEC_OK;
    if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    if (out_capacity < npx) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
    if (npx > 0xffffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "more than 2^32-1 pixels");
    HIP_TRY(hipSetDevice(q->dev.device));
    int rc;
    if ((rc = q->h2d.ensure(round_up4(n_bytes) + 16))) return rc;
    if ((rc = q->d2h.ensure(npx * sizeof(float)))) return rc;
    HIP_TRY(hipMemcpyAsync(q->h2d.p, blob, n_bytes, hipMemcpyHostToDevice, q->stream));
    // the header's width/height are ignored by the reference too: everything after byte 26 is one row of pixels
    QuantDesc d;
    uint32_t items, bpx, bdw;
    d = QuantDesc{};
    d.rows = 1; d.width = static_cast<uint32_t>(npx); d.n_images = 1; d.chunks = 1; d.chunk_w = d.width;
    d.header = kTgaHeader; d.vec = 1; d.img_out = static_cast<float *>(q->d2h.p); d.blob = static_cast<uint8_t *>(q->h2d.p);
    items = 1; bpx = 0; (void)bpx;
    bdw = static_cast<uint32_t>(((kTgaHeader + npx + 3) / 4 + kQuantDwPerBlock - 1) / kQuantDwPerBlock);
    hipLaunchKernelGGL(quant_decode_kernel, dim3(items * bdw), dim3(kQuantThreads), 0, q->stream, d, bdw);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, q->d2h.p, npx * sizeof(float), hipMemcpyDeviceToHost, q->stream));
    HIP_TRY(hipStreamSynchronize(q->stream));
    if (n_values) *n_values = npx;
    return MELSPEC_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// VAD column classification (vad_boundaries, src/vad.rs:256-340)
// ------------------------------------------------------------------------------------
extern "C" {

void melspec_vad_default_settings(melspec_vad_settings *s) {          // DetectionSettings::default, src/vad.rs:13-22
    if (!s) return;
    s->min_energy = 0.98; s->min_y = 11; s->min_x = 5; s->min_mel = 2;
}

size_t melspec_vad_mask_len(int n_mels, size_t width) { return (n_mels < 3 || width < 3) ? 0 : width - 2; }

int melspec_vad_boundaries_device(const float *d_images, size_t image_stride, int n_mels, size_t width, uint32_t n_images,
                                  const melspec_vad_settings *settings, uint8_t *d_raw, uint8_t *d_smoothed, size_t mask_stride,
                                  uint32_t *d_longest_run, void *stream) {
    if (!settings) return fail(MELSPEC_ERR_INVALID_ARG, "settings is NULL");
    if (n_mels < 0 || settings->min_y < 0 || settings->min_mel < 0) return fail(MELSPEC_ERR_INVALID_ARG, "negative size");
    const size_t n = melspec_vad_mask_len(n_mels, width);
    if (n_images == 0) return MELSPEC_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n == 0) {                                        // EdgeInfo::new(empty, empty), src/vad.rs:270-272
        if (d_longest_run) HIP_TRY(hipMemsetAsync(d_longest_run, 0, sizeof(uint32_t) * n_images, s));
        return MELSPEC_OK;
    }
    if (!d_images || !d_smoothed) return fail(MELSPEC_ERR_INVALID_ARG, "image/mask pointer is NULL");
    if (!d_raw) return fail(MELSPEC_ERR_INVALID_ARG, "d_raw is NULL (the vote reads the raw mask)");
    if (mask_stride < n) return fail(MELSPEC_ERR_INVALID_ARG, "mask_stride < width - 2");
    if (image_stride < static_cast<size_t>(n_mels) * width) return fail(MELSPEC_ERR_INVALID_ARG, "image_stride < n_mels * width");
    if (width > 0xffffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "image wider than 2^32-1 columns");
    VadDesc d{};
    d.img = d_images; d.raw = d_raw; d.smoothed = d_smoothed; d.longest = d_longest_run;
    d.img_stride = image_stride; d.mask_stride = mask_stride;
    d.height = static_cast<uint32_t>(n_mels); d.width = static_cast<uint32_t>(width); d.n_images = n_images;
    d.min_mel = settings->min_mel; d.min_y = settings->min_y; d.thr = settings->min_energy * settings->min_energy;
    const uint64_t bpi = (n + 255) / 256;
    if (bpi * n_images > 0x7fffffffull) return fail(MELSPEC_ERR_UNSUPPORTED, "batch too large for one launch");
    const unsigned grid = static_cast<unsigned>(bpi * n_images);
    hipLaunchKernelGGL(vad_raw_kernel, dim3(grid), dim3(256), 0, s, d, static_cast<uint32_t>(bpi), d_raw);
    hipLaunchKernelGGL(vad_smooth_kernel, dim3(grid), dim3(256), 0, s, d, static_cast<uint32_t>(bpi), d_raw);
    if (d_longest_run) hipLaunchKernelGGL(vad_run_kernel, dim3(n_images), dim3(64), 0, s, d);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_vad_boundaries_host(int device, const float *image, int n_mels, size_t width, const melspec_vad_settings *settings,
                                uint8_t *raw_out, uint8_t *smoothed_out, uint32_t *longest_run) {
    if (!settings) return fail(MELSPEC_ERR_INVALID_ARG, "settings is NULL");
    if (longest_run) *longest_run = 0;
    const size_t n = melspec_vad_mask_len(n_mels, width);
    if (n == 0) return MELSPEC_OK;
    if (!image || !smoothed_out) return fail(MELSPEC_ERR_INVALID_ARG, "image/out is NULL");
    DeviceInfo info;
    int rc = pick_device(device, info);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(info.device));
    DevBuf img, masks, run;
    const size_t px = static_cast<size_t>(n_mels) * width, ms = (n + 15) & ~static_cast<size_t>(15);
    auto done = [&](int code) { img.release(); masks.release(); run.release(); return code; };
    if ((rc = img.ensure(px * sizeof(float))) || (rc = masks.ensure(2 * ms)) || (rc = run.ensure(16))) return done(rc);
    if (hipMemcpy(img.p, image, px * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "hipMemcpy failed"));
    uint8_t *m = static_cast<uint8_t *>(masks.p);
    rc = melspec_vad_boundaries_device(static_cast<const float *>(img.p), px, n_mels, width, 1, settings, m, m + ms, ms,
                                       static_cast<uint32_t *>(run.p), nullptr);
    if (rc) return done(rc);
    if (hipDeviceSynchronize() != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "vad kernels failed"));
    if (raw_out && hipMemcpy(raw_out, m, n, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "hipMemcpy failed"));
    if (hipMemcpy(smoothed_out, m + ms, n, hipMemcpyDeviceToHost) != hipSuccess) return done(fail(MELSPEC_ERR_INTERNAL, "hipMemcpy failed"));
    if (longest_run && hipMemcpy(longest_run, run.p, sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess)
        return done(fail(MELSPEC_ERR_INTERNAL, "hipMemcpy failed"));
    return done(MELSPEC_OK);
}

}  // extern "C"

extern "C" {


static int synth_launch(float *d_out, uint64_t clip_stride, uint64_t first_sample, uint64_t n_samples, uint64_t first_clip,
                        uint32_t n_clips, uint32_t seed, void *stream) {
    if (n_clips == 0 || n_samples == 0) return MELSPEC_OK;
    if (!d_out) return fail(MELSPEC_ERR_INVALID_ARG, "d_out is NULL");
    const uint64_t total = static_cast<uint64_t>(n_clips) * n_samples;
    uint64_t blocks = (total + 255) / 256;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(synth_pcm_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       d_out, clip_stride, n_samples, first_clip, n_clips, seed, first_sample);
    HIP_TRY(hipGetLastError());
    return MELSPEC_OK;
}

int melspec_synth_pcm_device(float *d_out, uint64_t clip_stride, uint64_t clip_len, uint64_t first_clip,
                             uint32_t n_clips, uint32_t seed, void *stream) {
    return synth_launch(d_out, clip_stride, 0, clip_len, first_clip, n_clips, seed, stream);
}

int melspec_synth_pcm_window_device(float *d_out, uint64_t clip_stride, uint64_t first_sample, uint64_t n_samples,
                                    uint64_t first_clip, uint32_t n_clips, uint32_t seed, void *stream) {
    return synth_launch(d_out, clip_stride, first_sample, n_samples, first_clip, n_clips, seed, stream);
}

}  // extern "C"
