// stream_bank.hpp -- what the banks of live streams share on the host side: the Whisper bank (melspec_stream_*, aux.hip), the Kaldi
// fbank's (melspec_fbank_stream_*, fbank512.hip) and the NeMo / Parakeet frontend's (melspec_blm_stream_*, fbank512.hip) are this core plus
// their own planner (stream_plan.hpp / fbank_stream_plan.hpp / blm_stream_plan.hpp) and their own frame stage; the latter two, which also
// keep running statistics of their rows, are one bank written once on top of this core (stat_bank.hpp).  A bank is n_streams slots of `stride` floats in HBM, [carry, ending at in_off][next chunk at in_off]; a push is
//   entries up (unless the device still holds them) -> scatter -> the bank's frame stage -> carry -> wait
// on one stream, and the host form of it stages samples and rows through the bank's two buffers.
#pragma once
#include "host_common.hpp"

namespace melspec {
namespace host {

struct BankCore {
    int device = -1;
    hipStream_t stream = nullptr;        // the owning object's: the host calls and reset run on it
    DevBuf state, staging, out;          // [n_streams][stride] f32; the host calls' samples and rows
    RaggedScratch ring, plan_ring;       // per-push entry tables / ragged plans (the owning object's own ring serves its other callers)
    uint64_t stride = 0;
    uint32_t in_off = 0, n_streams = 0;
    float *slot(uint32_t id) const { return static_cast<float *>(state.p) + id * stride; }
};

// a planner's status (stream_plan_push, fbank_stream_plan_push, blm_stream_plan_push) as the ABI's
inline int plan_status(int rc, const char *err) {
    return rc == 1 ? fail(MELSPEC_ERR_INVALID_ARG, err) : rc == 2 ? fail(MELSPEC_ERR_CAPACITY, err) : MELSPEC_OK;
}

// A ring slot is in use by queued work from its upload on: every exit records its event (the next user of the slot waits for it).
struct SlotGuard { RaggedSlot *sl; hipStream_t s; ~SlotGuard() { plan_ragged_done(sl, s); } };

inline int core_create(BankCore &c, int device, hipStream_t stream, uint32_t n_streams, uint64_t stride, uint32_t in_off) {
    c.device = device; c.stream = stream; c.n_streams = n_streams; c.stride = stride; c.in_off = in_off;
    if (hipSetDevice(device) != hipSuccess) return fail(MELSPEC_ERR_UNAVAILABLE, "hipSetDevice failed");
    const size_t bytes = static_cast<size_t>(n_streams) * stride * sizeof(float) + 64;
    if (int rc = c.state.ensure(bytes)) return rc;
    if (hipMemset(c.state.p, 0, bytes) != hipSuccess) return fail(MELSPEC_ERR_INTERNAL, "hipMemset failed");
    return MELSPEC_OK;
}

inline void core_destroy(BankCore &c) {
    if (c.device >= 0) { (void)hipSetDevice(c.device); (void)hipStreamSynchronize(c.stream); }
    c.state.release(); c.staging.release(); c.out.release(); c.ring.release(); c.plan_ring.release();
}

// where a device producer writes stream id's next chunk
inline float *core_input_ptr(const BankCore &c, uint32_t id) { return id < c.n_streams ? c.slot(id) + c.in_off : nullptr; }

// Every id is checked before anything is touched; then the memsets of the slots' carries are queued on the bank's stream (ids NULL: of the
// whole state).  The caller resets what else it keeps per stream and waits for the stream.
inline int core_reset_slots(BankCore &c, const uint32_t *ids, uint32_t n) {
    for (uint32_t i = 0; ids && i < n; ++i)
        if (ids[i] >= c.n_streams) return fail(MELSPEC_ERR_INVALID_ARG, "stream id out of range");
    HIP_TRY(hipSetDevice(c.device));
    if (!ids) HIP_TRY(hipMemsetAsync(c.state.p, 0, static_cast<size_t>(c.n_streams) * c.stride * sizeof(float), c.stream));
    for (uint32_t i = 0; ids && i < n; ++i) HIP_TRY(hipMemsetAsync(c.slot(ids[i]), 0, c.in_off * sizeof(float), c.stream));
    return MELSPEC_OK;
}

// where a push reads and writes
struct PushArgs {
    const void *d_src;               // the chunks (NULL: already in the slots, at core_input_ptr)
    int pcm_dtype;                   // their element type: the scatter converts into the f32 state
    const uint64_t *h_src_off;       // where they start in d_src, in elements (NULL: back to back, the plan's own offsets)
    void *d_out;
    const uint64_t *h_out_off;       // caller-placed rows (NULL: packed, the plan's own offsets); the stages behind the frames read them there
    hipStream_t stream;
    bool zero_fill = false;          // an entry appends zeros to its stream (a flush): the scatter runs without a source, too
};

// The entries and, behind them, a table of the bank's own (`tail`) travel like a ragged plan: pinned slot, copy kernel on the launch stream.
inline int core_upload_entries(BankCore &c, const StreamEntry *entries, uint32_t n, const PushArgs &a, const void *tail, size_t tail_bytes, SlotGuard &guard,
                               const StreamEntry *&d_e, const void *&d_tail) {
    const size_t ebytes = round16(static_cast<size_t>(n) * sizeof(StreamEntry)), bytes = ebytes + round16(tail_bytes);
    RaggedSlot *sl = nullptr;
    if (int rc = table_slot_take(c.ring, bytes, sl)) return rc;
    StreamEntry *h_e = static_cast<StreamEntry *>(sl->host);
    std::memcpy(h_e, entries, static_cast<size_t>(n) * sizeof(StreamEntry));
    for (uint32_t i = 0; i < n && a.h_out_off; ++i) h_e[i].out_off = a.h_out_off[i];
    for (uint32_t i = 0; i < n && a.h_src_off; ++i) h_e[i].src_off = a.h_src_off[i];
    if (tail_bytes) std::memcpy(static_cast<char *>(sl->host) + ebytes, tail, tail_bytes);
    guard.sl = sl;
    if (int rc = table_slot_upload(*sl, bytes, a.stream)) return rc;
    d_e = static_cast<const StreamEntry *>(sl->dev.p);
    d_tail = static_cast<const char *>(sl->dev.p) + ebytes;
    return MELSPEC_OK;
}

// One push on a.stream.  cached_d_e: the device still holds the entries (the push repeats the one that left them there): no upload.
// frames(d_e, d_tail) queues the bank's frame stage; it is called when the push emits a row.  The contract of the push calls: the
// launches have completed on return (a device producer may refill its slot at once).
template <class Frames>
int core_run(BankCore &c, const StreamEntry *entries, uint32_t n, uint64_t total_frames, const PushArgs &a, const StreamEntry *cached_d_e, const void *tail,
             size_t tail_bytes, Frames frames) {
    if (total_frames && !a.d_out) return fail(MELSPEC_ERR_INVALID_ARG, "d_out is NULL");      // before anything is queued
    HIP_TRY(hipSetDevice(c.device));
    SlotGuard guard{nullptr, a.stream};
    const StreamEntry *d_e = cached_d_e;
    const void *d_tail = nullptr;
    int rc;
    if (!d_e && (rc = core_upload_entries(c, entries, n, a, tail, tail_bytes, guard, d_e, d_tail))) return rc;
    float *state = static_cast<float *>(c.state.p);
    if ((a.d_src || a.zero_fill) && (rc = stream_scatter_launch(state, c.stride, c.in_off, d_e, n, a.d_src, a.pcm_dtype, a.stream))) return rc;
    if (total_frames && (rc = frames(d_e, d_tail))) return rc;
    if ((rc = stream_carry_launch(state, c.stride, c.in_off, d_e, n, a.stream))) return rc;
    HIP_TRY(hipStreamSynchronize(a.stream));
    return MELSPEC_OK;
}

// the host form's ends
struct HostPush {
    const void *samples;             // the entries' chunks back to back
    void *out;
    size_t out_capacity;             // in elements
    uint64_t need;                   // elements the push emits
    size_t sample_bytes, elem_bytes; // per sample, per element
};

// Samples up through `staging`, run(d_src, d_out, stream) -- a core_run --, rows down through `out`; synchronous.
template <class Run>
int core_push_host(BankCore &c, const StreamEntry *entries, uint32_t n, const HostPush &h, Run run) {
    if (h.need > h.out_capacity) return fail(MELSPEC_ERR_CAPACITY, "output buffer too small");
    if (h.need && !h.out) return fail(MELSPEC_ERR_INVALID_ARG, "out is NULL");
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) total += entries[i].len;
    if (total && !h.samples) return fail(MELSPEC_ERR_INVALID_ARG, "samples is NULL");
    HIP_TRY(hipSetDevice(c.device));
    int rc;
    if ((rc = c.staging.ensure(total * h.sample_bytes + 16)) || (rc = c.out.ensure(h.need * h.elem_bytes + 16))) return rc;
    if (total) HIP_TRY(hipMemcpyAsync(c.staging.p, h.samples, total * h.sample_bytes, hipMemcpyHostToDevice, c.stream));
    if ((rc = run(total ? c.staging.p : nullptr, c.out.p, c.stream))) return rc;
    if (h.need) {
        HIP_TRY(hipMemcpyAsync(h.out, c.out.p, h.need * h.elem_bytes, hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipStreamSynchronize(c.stream));
    }
    return MELSPEC_OK;
}

}  // namespace host
}  // namespace melspec
