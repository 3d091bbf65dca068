// blm_stream_plan.hpp -- host bookkeeping of the NeMo / Parakeet frontend's stream bank (plain C++, no HIP): which columns of
// BatchLogMelSpectrogram::compute (compute_flat_with_scratch, num_frames, prepare_padded_waveform, apply_preemphasis in src/mel.rs) a push
// completes and where their samples start in the bank's state.  Shared by fbank512.hip (the NeMo traits of stat_bank.hpp's StatBank, which
// is the bank around this planner) and tests/cpp/blm_stream_host.cpp.  The plan's `len` and `org0` go to the device as the bank's own tail
// (stat_bank_tail.hpp).
//
// Frame k of a clip reads the 400 window taps from sample k * hop + org0 on (org0 = -200 centred: the window sits in the middle of the
// 512-point frame whose centre is sample k * hop; +56 otherwise) and, for the pre-emphasis of its first tap, the sample in front of them.
// A push emits frame k once every one of its taps is a real sample: the stream holds k * hop + org0 + 400 samples.  A centred clip of
// `total` samples has total / hop + 1 frames, the last ones reading zeros behind the clip: those are what finish emits, and they depend on
// where the clip ends.  Not centred, num_frames asks for the whole 512-point frame (k * hop + 512 samples) and there is nothing to finish.
// Slot layout (as stream_plan.hpp's): [carry, right-aligned so that it ends at in_off][next chunk at in_off, <= max_chunk].  With E frames
// emitted the carry holds the stream's samples from b = max(0, E * hop + org0 - 1) on -- the predecessor of the next frame's first tap, then
// everything behind it (from `total` on when the stream has not reached b yet: what lies before b is never read again).  While b = 0 the
// clip of the push starts at the stream's sample 0 and the kernel's guarded form supplies the left padding and the unemphasised first
// sample; afterwards index 0 of the clip is only ever read as a predecessor.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "stream_plan.hpp"

namespace melspec {

constexpr uint32_t kBlmStreamTaps = 400;         // win_length of the fused geometry
constexpr uint32_t kBlmStreamFft = 512;

struct BlmStreamGeom {
    uint32_t hop, n_mels, n_streams, max_chunk;
    int32_t org0;         // first tap of frame 0: -200 centred, +56 not
    bool center;
    uint32_t in_off;      // carry capacity: the carry is shorter than 401 samples centred and 457 not; multiple of 4
    uint64_t stride;      // floats per slot
};

inline BlmStreamGeom blm_stream_geometry(uint32_t hop, bool center, uint32_t n_mels, uint32_t n_streams, uint32_t max_chunk) {
    BlmStreamGeom g{};
    g.hop = hop; g.n_mels = n_mels; g.n_streams = n_streams; g.max_chunk = max_chunk; g.center = center;
    g.org0 = center ? -static_cast<int32_t>(kBlmStreamTaps / 2) : static_cast<int32_t>((kBlmStreamFft - kBlmStreamTaps) / 2);
    g.in_off = ((center ? kBlmStreamTaps + 1u : kBlmStreamFft - (kBlmStreamFft - kBlmStreamTaps) / 2 + 1u) + 3u) & ~3u;      // 404 / 460
    g.stride = (static_cast<uint64_t>(g.in_off) + max_chunk + 7) & ~static_cast<uint64_t>(3);
    return g;
}

struct BlmStreamBook : PushMarks {
    std::vector<uint64_t> total;         // samples received
    std::vector<uint64_t> emitted;       // columns emitted (E)
    std::vector<uint8_t> ended;          // finished: no push until a reset
    void reset(uint32_t n) { total.assign(n, 0); emitted.assign(n, 0); ended.assign(n, 0); PushMarks::reset(n); }
    void reset_one(uint32_t s) { total[s] = 0; emitted[s] = 0; ended[s] = 0; }
};

struct BlmStreamPlan {
    std::vector<StreamEntry> entries;          // what the scatter / carry / statistics kernels read (zero_fill and act_base stay 0)
    std::vector<uint64_t> off, out_off;        // ragged batch over the state buffer: the clip's sample 0 (the stream's sample b), output offset
    std::vector<uint64_t> frames;
    std::vector<uint64_t> len;                 // samples of the clip: what the slot holds from b on
    std::vector<int32_t> org0;                 // the clip's own window origin: first tap of its first frame
    uint64_t total_frames = 0;
};

// frames of a stream that has received n samples and goes on: every tap a real sample
inline uint64_t blm_stream_frames(const BlmStreamGeom &g, uint64_t n) {
    const uint64_t need = g.center ? kBlmStreamTaps / 2 : kBlmStreamFft;
    return n < need ? 0 : 1 + (n - need) / g.hop;
}
// num_frames (src/mel.rs) of a clip that ends at n samples
inline uint64_t blm_stream_frames_ended(const BlmStreamGeom &g, uint64_t n) {
    if (!g.center) return blm_stream_frames(g, n);
    return n == 0 ? 0 : n / g.hop + 1;
}
// first sample the slot still needs with e frames emitted (before the cap at `total`)
inline uint64_t blm_stream_base(const BlmStreamGeom &g, uint64_t e) {
    const int64_t b = static_cast<int64_t>(e * g.hop) + g.org0 - 1;
    return b < 0 ? 0 : static_cast<uint64_t>(b);
}

// returns 0 ok, 1 invalid argument, 2 capacity; *err names the problem.  The book is not changed (blm_stream_commit_push does that).
// finish: a push of no samples that emits the frames which read past the stream's end (lens is not read).
inline int blm_stream_plan_push(const BlmStreamGeom &g, BlmStreamBook &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool finish,
                                BlmStreamPlan &pl, const char **err) {
    pl.entries.resize(n); pl.off.resize(n); pl.out_off.resize(n); pl.frames.resize(n); pl.len.resize(n); pl.org0.resize(n);
    PushAdmission adm(bk, g.n_streams, g.max_chunk, g.n_mels);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i], len = finish ? 0 : lens[i];
        StreamEntry &e = pl.entries[i];
        if (const int rc = adm.admit(s, len, e, err)) return rc;
        if (bk.ended[s]) { *err = finish ? "the stream is already finished (reset starts it afresh)" : "push to a finished stream (reset starts it afresh)"; return 1; }
        const uint64_t total0 = bk.total[s], total1 = total0 + len, e0 = bk.emitted[s];
        const uint64_t e1 = finish ? blm_stream_frames_ended(g, total1) : blm_stream_frames(g, total1);
        const uint64_t b0 = blm_stream_base(g, e0), held0 = std::min(b0, total0);          // the carry holds [held0, total0)
        const uint32_t keep0 = static_cast<uint32_t>(total0 - held0);
        adm.place(e, e1 - e0);
        pl.frames[i] = e1 - e0;
        pl.off[i] = static_cast<uint64_t>(s) * g.stride + g.in_off - keep0 + (b0 - held0);
        pl.len[i] = total1 > b0 ? total1 - b0 : 0;
        pl.org0[i] = static_cast<int32_t>(static_cast<int64_t>(e0 * g.hop) + g.org0 - static_cast<int64_t>(b0));
        pl.out_off[i] = e.out_off;
        // the carry after the push: from b' on (a finished stream keeps what it has: nothing reads it again)
        const uint64_t b1 = blm_stream_base(g, e1);
        e.keep = finish ? keep0 : static_cast<uint32_t>(total1 - std::min(b1, total1));
    }
    pl.total_frames = adm.total_frames();
    return 0;
}

inline void blm_stream_commit_push(const BlmStreamGeom &g, BlmStreamBook &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool finish) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i];
        if (finish) { bk.emitted[s] = blm_stream_frames_ended(g, bk.total[s]); bk.ended[s] = 1; continue; }
        bk.total[s] += lens[i];
        bk.emitted[s] = blm_stream_frames(g, bk.total[s]);
    }
}

inline size_t blm_stream_frames_after(const BlmStreamGeom &g, const BlmStreamBook &bk, uint32_t id, uint32_t n_new) {
    return bk.ended[id] ? 0 : static_cast<size_t>(blm_stream_frames(g, bk.total[id] + n_new) - bk.emitted[id]);
}
inline size_t blm_stream_finish_frames(const BlmStreamGeom &g, const BlmStreamBook &bk, uint32_t id) {
    return bk.ended[id] ? 0 : static_cast<size_t>(blm_stream_frames_ended(g, bk.total[id]) - bk.emitted[id]);
}

}  // namespace melspec
