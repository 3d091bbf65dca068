// fbank_stream_plan.hpp -- host bookkeeping of the Kaldi fbank's stream bank (plain C++, no HIP): which frames of Fbank::compute
// (src/fbank.rs:141-236) a push completes and where their samples start in the bank's state.  Shared by fbank512.hip (the Kaldi traits of
// stat_bank.hpp's StatBank, which is the bank around this planner) and tests/cpp/fbank_stream_host.cpp.  The plan's `continues` goes to
// the device as the bank's own tail (stat_bank_tail.hpp).
//
// A stream that has received `total` samples has emitted E = frames(total) rows (src/fbank.rs:147-151: 0 below frame_len, then one per
// shift) -- the first rows of Fbank::compute on whatever the stream goes on to receive, since a row depends on its own frame_len samples and
// the one in front of them only.  No warm-up, no flush: the reference drops the tail.
// Slot layout (as stream_plan.hpp's): [carry, right-aligned so that it ends at in_off][next chunk at in_off, <= max_chunk].  The carry holds
// the samples from E * shift - 1 on: the predecessor of the next frame's first sample (src/fbank.rs:177-181; only when E > 0 -- a stream
// that has emitted nothing has none, and what lies in front of its samples is never read), then the total - E * shift < frame_len samples
// that no emitted frame starts in.  Needs shift <= frame_len.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "stream_plan.hpp"

namespace melspec {

struct FbankStreamGeom {
    uint32_t frame_len, shift, n_mels, n_streams, max_chunk;
    uint32_t in_off;      // carry capacity: >= frame_len + 1 (the predecessor, then at most frame_len - 1 samples, rounded generously), multiple of 4
    uint64_t stride;      // floats per slot
};

inline FbankStreamGeom fbank_stream_geometry(uint32_t frame_len, uint32_t shift, uint32_t n_mels, uint32_t n_streams, uint32_t max_chunk) {
    FbankStreamGeom g{};
    g.frame_len = frame_len; g.shift = shift; g.n_mels = n_mels; g.n_streams = n_streams; g.max_chunk = max_chunk;
    g.in_off = (frame_len + 1u + 3u) & ~3u;
    g.stride = (static_cast<uint64_t>(g.in_off) + max_chunk + 7) & ~static_cast<uint64_t>(3);
    return g;
}

struct FbankStreamBook : PushMarks {
    std::vector<uint64_t> total;         // samples received
    std::vector<uint64_t> emitted;       // rows emitted: frames(total)
    std::vector<uint32_t> pending;       // total - emitted * shift: the samples in the carry behind the predecessor (< frame_len)
    void reset(uint32_t n) { total.assign(n, 0); emitted.assign(n, 0); pending.assign(n, 0); PushMarks::reset(n); }
    void reset_one(uint32_t s) { total[s] = 0; emitted[s] = 0; pending[s] = 0; }
};

struct FbankStreamPlan {
    std::vector<StreamEntry> entries;          // what the scatter / carry / column-sum kernels read (zero_fill and act_base stay 0)
    std::vector<uint64_t> off, out_off;        // ragged batch over the state buffer: first sample of the entry's first frame, output offset
    std::vector<uint64_t> frames;
    std::vector<uint32_t> continues;           // the entry's first frame has a predecessor sample (the stream has emitted before)
    uint64_t total_frames = 0;
};

// src/fbank.rs:147-151
inline uint64_t fbank_stream_frames(const FbankStreamGeom &g, uint64_t n) { return n < g.frame_len ? 0 : 1 + (n - g.frame_len) / g.shift; }

// returns 0 ok, 1 invalid argument, 2 capacity; *err names the problem.  The book is not changed (fbank_stream_commit_push does that).
inline int fbank_stream_plan_push(const FbankStreamGeom &g, FbankStreamBook &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n,
                                  FbankStreamPlan &pl, const char **err) {
    pl.entries.resize(n); pl.off.resize(n); pl.out_off.resize(n); pl.frames.resize(n); pl.continues.resize(n);
    PushAdmission adm(bk, g.n_streams, g.max_chunk, g.n_mels);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i], len = lens[i];
        StreamEntry &e = pl.entries[i];
        if (const int rc = adm.admit(s, len, e, err)) return rc;
        const uint64_t e0 = bk.emitted[s], e1 = fbank_stream_frames(g, bk.total[s] + len);
        adm.place(e, e1 - e0);
        pl.frames[i] = e1 - e0;
        pl.continues[i] = e0 > 0 ? 1u : 0u;
        pl.off[i] = static_cast<uint64_t>(s) * g.stride + g.in_off - bk.pending[s];          // sample e0 * shift of the stream
        pl.out_off[i] = e.out_off;
        // the carry after the push: the samples from e1 * shift on and, once a frame has been emitted, the one in front of them
        e.keep = static_cast<uint32_t>(bk.total[s] + len - e1 * g.shift) + (e1 > 0 ? 1u : 0u);
    }
    pl.total_frames = adm.total_frames();
    return 0;
}

inline void fbank_stream_commit_push(const FbankStreamGeom &g, FbankStreamBook &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i];
        bk.total[s] += lens[i];
        bk.emitted[s] = fbank_stream_frames(g, bk.total[s]);
        bk.pending[s] = static_cast<uint32_t>(bk.total[s] - bk.emitted[s] * g.shift);
    }
}

inline size_t fbank_stream_frames_after(const FbankStreamGeom &g, const FbankStreamBook &bk, uint32_t id, uint32_t n_new) {
    return static_cast<size_t>(fbank_stream_frames(g, bk.total[id] + n_new) - bk.emitted[id]);
}

}  // namespace melspec
