// stat_bank.hpp -- a stream bank that keeps running statistics of the rows it emits, written once: the Kaldi fbank's bank
// (melspec_fbank_stream_*) and the NeMo / Parakeet frontend's (melspec_blm_stream_*) are StatBank<B> over stream_bank.hpp's core, and
// their extern "C" functions in fbank512.hip forward here.  B, the bank's traits (fbank512.hip, next to the objects they read), says
// what differs:
//   Owner, Geom, Book, Plan          the object the bank stands on; the planner's types (fbank_stream_plan.hpp / blm_stream_plan.hpp)
//   kMagic, kAccWords, kStats        the handle's tag; f64 words of running state per stream and bin; f32 arrays a stats call writes
//   kBankNull, kOwnerNull, kChunksNull, kStatsDeviceNull, kStatsHostNull      the messages that name the bank
//   ok(owner), supported(owner)      whether a bank can stand on the object; MELSPEC_OK, or the refusal with its message
//   geometry(owner, n_streams, max_chunk), plan(..., finish, pl, &err), commit(..., finish), frames_after(geom, book, id, n_new)
//   own_tail(pl, n)                  the table the frame stage reads behind the entries (stat_bank_tail.hpp)
//   frames(bank, bp, d_tail, n, s)   the frame stage over the ragged plan bp
//   fold(bank, d_e, src_off, rows, dst, out_dtype, n, s)      the rows into the running state; 16-bit rows: read at src_off, written to dst
//   read_out(bank, d_ids, n, out, s) the stats kernel
// The owner has dev.device, dev.cus and stream.
#pragma once
#include "stat_bank_tail.hpp"
#include "stream_bank.hpp"

namespace melspec {
namespace host {

template <class B>
struct StatBank {
    using Plan = typename B::Plan;

    uint32_t magic = B::kMagic;          // the handle crosses the ABI as void *: every call checks what it was given
    typename B::Owner *owner = nullptr;  // geometry, tables, kernels; not owned
    typename B::Geom geom{};
    typename B::Book book;               // the host side of the state
    BankCore core;
    DevBuf acc, counts;                  // [n_streams][kAccWords][n_mels] f64, [n_streams] u64
    DevBuf readout;                      // the host stats call's buffer
    DevBuf rows32;                       // the f32 rows of a push with 16-bit rows, packed in entry order: allocated by the first such push

    size_t acc_row() const { return static_cast<size_t>(geom.n_mels) * B::kAccWords * sizeof(double); }
    static constexpr size_t kCount = sizeof(unsigned long long);
    // the stats kernel's grid: a thread per stream and bin
    dim3 stats_grid(uint32_t n, int threads) const { return dim3(grid_for((static_cast<uint64_t>(n) * geom.n_mels + threads - 1) / threads, owner->dev.cus, 8)); }

    static StatBank *of(void *h) {
        StatBank *st = static_cast<StatBank *>(h);
        return st && st->magic == B::kMagic ? st : nullptr;
    }
    static const StatBank *of(const void *h) { return of(const_cast<void *>(h)); }

    static int create(void **out, typename B::Owner *owner, uint32_t n_streams, uint32_t max_chunk) {
        if (!out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
        *out = nullptr;
        if (n_streams == 0 || max_chunk == 0) return fail(MELSPEC_ERR_INVALID_ARG, "n_streams and max_chunk must be > 0");
        if (!owner) return fail(MELSPEC_ERR_INVALID_ARG, B::kOwnerNull);
        if (int rc = B::supported(owner)) return rc;
        StatBank *st = new (std::nothrow) StatBank();
        if (!st) return fail(MELSPEC_ERR_INTERNAL, "out of host memory");
        st->owner = owner;
        st->geom = B::geometry(owner, n_streams, max_chunk);
        st->book.reset(n_streams);
        auto bail = [&](int code) { destroy(st); return code; };
        const size_t acc_bytes = n_streams * st->acc_row(), count_bytes = n_streams * kCount;
        int rc;
        if ((rc = core_create(st->core, owner->dev.device, owner->stream, n_streams, st->geom.stride, st->geom.in_off)) || (rc = st->acc.ensure(acc_bytes)) ||
            (rc = st->counts.ensure(count_bytes)))
            return bail(rc);
        if (hipMemset(st->acc.p, 0, acc_bytes) != hipSuccess || hipMemset(st->counts.p, 0, count_bytes) != hipSuccess) return bail(fail(MELSPEC_ERR_INTERNAL, "hipMemset failed"));
        *out = st;
        return MELSPEC_OK;
    }

    static void destroy(void *h) {
        StatBank *st = of(h);
        if (!st) return;
        core_destroy(st->core);
        st->acc.release(); st->counts.release(); st->readout.release(); st->rows32.release();
        st->magic = 0;
        delete st;
    }

    static int reset(void *h, const uint32_t *ids, uint32_t n) {
        StatBank *st = of(h);
        if (!st) return fail(MELSPEC_ERR_INVALID_ARG, B::kBankNull);
        if (int rc = core_reset_slots(st->core, ids, n)) return rc;      // a bad id: nothing has been touched
        hipStream_t s = st->core.stream;
        const size_t row = st->acc_row(), n_streams = st->geom.n_streams;
        if (!ids) {
            HIP_TRY(hipMemsetAsync(st->acc.p, 0, n_streams * row, s));
            HIP_TRY(hipMemsetAsync(st->counts.p, 0, n_streams * kCount, s));
            st->book.reset(st->geom.n_streams);
        }
        for (uint32_t i = 0; ids && i < n; ++i) {
            HIP_TRY(hipMemsetAsync(static_cast<char *>(st->acc.p) + ids[i] * row, 0, row, s));
            HIP_TRY(hipMemsetAsync(static_cast<char *>(st->counts.p) + ids[i] * kCount, 0, kCount, s));
            st->book.reset_one(ids[i]);
        }
        HIP_TRY(hipStreamSynchronize(s));
        return MELSPEC_OK;
    }

    static size_t frames_after(const void *h, uint32_t id, uint32_t n_new) {
        const StatBank *st = of(h);
        return st && id < st->geom.n_streams ? B::frames_after(st->geom, st->book, id, n_new) : 0;
    }

    static float *input_ptr(void *h, uint32_t id) {
        StatBank *st = of(h);
        return st ? core_input_ptr(st->core, id) : nullptr;
    }

    static int supports_io(const void *h, int pcm_dtype, int out_dtype) {
        const StatBank *st = of(h);
        return st && io_pcm_known(pcm_dtype) && io_out_known(out_dtype) && B::ok(st->owner) ? 1 : 0;      // push_args, without its messages
    }

    // The frame stage behind the core's scatter, then the fold of its rows into the running state.  out_dtype: the row type at a.d_out.
    // 16-bit rows: the same frame stage, planned onto the bank's f32 scratch with the plan's packed offsets, and the typed twin of the
    // fold, which reads the rows there and writes the caller's (the scratch grows before anything is queued).
    int run(const Plan &pl, uint32_t n, const PushArgs &a, int out_dtype) {
        const uint32_t nm = geom.n_mels;
        const bool typed = out_dtype != MELSPEC_OUT_F32;
        const std::vector<unsigned char> own = B::own_tail(pl, n);
        TypedTail tail(own.data(), own.size(), typed ? pl.out_off.data() : nullptr, n);
        if (typed && pl.total_frames) {
            if (!a.d_out) return fail(MELSPEC_ERR_INVALID_ARG, "d_out is NULL");
            HIP_TRY(hipSetDevice(core.device));
            if (int rc = rows32.ensure(static_cast<size_t>(pl.total_frames) * nm * sizeof(float) + 16)) return rc;
        }
        float *rows = static_cast<float *>(typed ? rows32.p : a.d_out);
        const uint64_t *rows_off = a.h_out_off && !typed ? a.h_out_off : pl.out_off.data();
        return core_run(core, pl.entries.data(), n, pl.total_frames, a, nullptr, tail.data, tail.bytes, [&](const StreamEntry *d_e, const void *d_tail) {
            BatchPlan bp;
            RaggedSlot *pslot = nullptr;
            int rc = plan_ragged(core.plan_ring, a.stream, static_cast<float *>(core.state.p), rows, pl.off.data(), pl.frames, rows_off, n, static_cast<int>(nm), kFbFPW, bp, pslot);
            if (!rc) rc = B::frames(*this, bp, d_tail, n, a.stream);
            plan_ragged_done(pslot, a.stream);
            if (rc) return rc;
            HIP_TRY(B::fold(*this, d_e, typed ? tail.packed_on_device(d_tail) : nullptr, rows, a.d_out, out_dtype, n, a.stream));
            return static_cast<int>(MELSPEC_OK);
        });
    }

    // what every push checks first: the handle, the dtype codes, the object
    static int push_args(StatBank *st, int pcm_dtype, int out_dtype) {
        if (!st) return fail(MELSPEC_ERR_INVALID_ARG, B::kBankNull);
        int io;
        if (int rc = io_dtypes(pcm_dtype, out_dtype, io)) return rc;
        return B::supported(st->owner);
    }
    // ... and, with something to do, the tables (a finish reads no lens)
    static int push_tables(const uint32_t *ids, const uint32_t *lens, bool finish) {
        if (!ids) return fail(MELSPEC_ERR_INVALID_ARG, finish ? "ids is NULL" : "ids/lens is NULL");
        if (!finish && !lens) return fail(MELSPEC_ERR_INVALID_ARG, "ids/lens is NULL");
        return MELSPEC_OK;
    }

    // a push or a finish behind its argument checks: plan, run(plan) -- its launches have completed when it returns --, then the book moves on
    template <class Run>
    int push(const uint32_t *ids, const uint32_t *lens, uint32_t n, bool finish, uint32_t *frames_out, Run run_plan) {
        Plan pl;
        const char *err = nullptr;
        int rc = plan_status(B::plan(geom, book, ids, lens, n, finish, pl, &err), err);
        if (rc || (rc = run_plan(pl))) return rc;
        B::commit(geom, book, ids, lens, n, finish);
        for (uint32_t i = 0; frames_out && i < n; ++i) frames_out[i] = static_cast<uint32_t>(pl.frames[i]);
        return MELSPEC_OK;
    }

    // *_push_host / _finish_host and their _io forms (finish: no samples, lens is not read): the rows cross the bus in their own type
    static int push_host(void *h, const uint32_t *ids, const void *samples, int pcm_dtype, const uint32_t *lens, uint32_t n, bool finish, void *out, int out_dtype,
                         size_t out_capacity_elems, uint32_t *frames_out) {
        StatBank *st = of(h);
        if (int rc = push_args(st, pcm_dtype, out_dtype)) return rc;
        if (n == 0) return MELSPEC_OK;
        if (int rc = push_tables(ids, lens, finish)) return rc;
        return st->push(ids, lens, n, finish, frames_out, [&](const Plan &pl) {
            const HostPush hp{samples, out, out_capacity_elems, pl.total_frames * static_cast<uint64_t>(st->geom.n_mels), io_pcm_bytes(pcm_dtype), io_out_bytes(out_dtype)};
            return core_push_host(st->core, pl.entries.data(), n, hp, [&](const void *d_src, void *d_out, hipStream_t s) {
                return st->run(pl, n, PushArgs{d_src, pcm_dtype, nullptr, d_out, nullptr, s}, out_dtype);
            });
        });
    }

    // *_push_device / _finish_device and their _io forms (finish: d_chunks NULL, MELSPEC_PCM_F32, lens is not read)
    static int push_device(void *h, const uint32_t *ids, const void *d_chunks, int pcm_dtype, const uint64_t *h_src_offsets, const uint32_t *lens, uint32_t n, bool finish,
                           void *d_out, int out_dtype, const uint64_t *h_out_offsets, uint32_t *frames_out, void *stream) {
        StatBank *st = of(h);
        if (int rc = push_args(st, pcm_dtype, out_dtype)) return rc;
        if (n == 0) return MELSPEC_OK;
        if (int rc = push_tables(ids, lens, finish)) return rc;
        if (!finish && !d_chunks && pcm_dtype != MELSPEC_PCM_F32) return fail(MELSPEC_ERR_INVALID_ARG, B::kChunksNull);
        if (io_misaligned(d_chunks, d_out, pcm_dtype | out_dtype << 4)) return fail(MELSPEC_ERR_INVALID_ARG, "device pointer is not aligned to its element type");
        return st->push(ids, lens, n, finish, frames_out, [&](const Plan &pl) {
            return st->run(pl, n, PushArgs{d_chunks, pcm_dtype, d_chunks ? h_src_offsets : nullptr, d_out, h_out_offsets,
                                           stream ? static_cast<hipStream_t>(stream) : st->core.stream}, out_dtype);
        });
    }

    // out: kStats device arrays of [n][n_mels] f32
    static int stats_device(void *h, const uint32_t *ids, uint32_t n, float *const *out, uint64_t *h_counts, void *stream) {
        StatBank *st = of(h);
        if (!st) return fail(MELSPEC_ERR_INVALID_ARG, B::kBankNull);
        if (n == 0) return MELSPEC_OK;
        if (!ids) return fail(MELSPEC_ERR_INVALID_ARG, "ids is NULL");
        for (int k = 0; k < B::kStats; ++k)
            if (!out[k]) return fail(MELSPEC_ERR_INVALID_ARG, B::kStatsDeviceNull);
        for (uint32_t i = 0; i < n; ++i)
            if (ids[i] >= st->geom.n_streams) return fail(MELSPEC_ERR_INVALID_ARG, "stream id out of range");
        HIP_TRY(hipSetDevice(st->core.device));
        hipStream_t s = stream ? static_cast<hipStream_t>(stream) : st->core.stream;
        const size_t bytes = round16(static_cast<size_t>(n) * sizeof(uint32_t));
        RaggedSlot *sl = nullptr;
        int rc = table_slot_take(st->core.ring, bytes, sl);
        if (rc) return rc;
        std::memcpy(sl->host, ids, static_cast<size_t>(n) * sizeof(uint32_t));
        SlotGuard slot_guard{sl, s};
        if ((rc = table_slot_upload(*sl, bytes, s))) return rc;
        B::read_out(*st, static_cast<const uint32_t *>(sl->dev.p), n, out, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        if (h_counts)
            for (uint32_t i = 0; i < n; ++i) h_counts[i] = st->book.emitted[ids[i]];
        return MELSPEC_OK;
    }

    // out: kStats host arrays; staged through `readout`, one behind the other
    static int stats_host(void *h, const uint32_t *ids, uint32_t n, float *const *out, uint64_t *counts) {
        StatBank *st = of(h);
        if (!st) return fail(MELSPEC_ERR_INVALID_ARG, B::kBankNull);
        if (n == 0) return MELSPEC_OK;
        for (int k = 0; k < B::kStats; ++k)
            if (!out[k]) return fail(MELSPEC_ERR_INVALID_ARG, B::kStatsHostNull);
        HIP_TRY(hipSetDevice(st->core.device));
        const size_t elems = static_cast<size_t>(n) * st->geom.n_mels, bytes = elems * sizeof(float);
        if (int rc = st->readout.ensure(B::kStats * bytes + 16)) return rc;
        float *d_out[B::kStats];
        for (int k = 0; k < B::kStats; ++k) d_out[k] = static_cast<float *>(st->readout.p) + k * elems;
        if (int rc = stats_device(h, ids, n, d_out, counts, st->core.stream)) return rc;
        for (int k = 0; k < B::kStats; ++k) HIP_TRY(hipMemcpy(out[k], d_out[k], bytes, hipMemcpyDeviceToHost));
        return MELSPEC_OK;
    }
};

}  // namespace host
}  // namespace melspec
