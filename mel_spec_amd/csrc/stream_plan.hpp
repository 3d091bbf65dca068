// stream_plan.hpp -- host bookkeeping of the streaming bank (plain C++, no HIP): which frames a push emits
// and where they start, restating Spectrogram::add (src/stft.rs:48-86) driven hop by hop the way
// RingBuffer::maybe_mel does (src/rb.rs:86-121); what every stream bank's planner shares (the admission of a push's entries, fbank_stream_plan.hpp
// is the other caller); and the key under which the bank keeps its last plan for the pushes that repeat it.  Shared by aux.hip,
// tests/emu and tests/cpp.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace melspec {

// Slot layout: [carry, right-aligned so that it ends at in_off][next chunk at in_off, <= max_chunk (+ < hop zeros on flush)].
struct StreamGeom {
    uint32_t n_fft, hop, n_mels, n_streams, max_chunk;
    uint32_t in_off;      // carry capacity: >= n_fft - 1 (history n_fft - hop, pending < hop), multiple of 4
    uint64_t stride;      // floats per slot
};

inline StreamGeom stream_geometry(uint32_t n_fft, uint32_t hop, uint32_t n_mels, uint32_t n_streams, uint32_t max_chunk) {
    StreamGeom g{};
    g.n_fft = n_fft; g.hop = hop; g.n_mels = n_mels; g.n_streams = n_streams; g.max_chunk = max_chunk;
    g.in_off = (n_fft + 3u) & ~3u;
    g.stride = (static_cast<uint64_t>(g.in_off) + max_chunk + hop + 7) & ~static_cast<uint64_t>(3);
    return g;
}

struct PushMarks {                       // duplicate detection inside one push: mark[s] == epoch once stream s has been admitted to it
    std::vector<uint32_t> mark;
    uint32_t epoch = 0;
    void reset(uint32_t n) { mark.assign(n, 0); epoch = 0; }
};

struct StreamBook : PushMarks {
    std::vector<uint32_t> pending;       // RingBuffer::accumulated_samples.len()
    std::vector<uint64_t> idx;           // Spectrogram::idx
    void reset(uint32_t n) { pending.assign(n, 0); idx.assign(n, 0); PushMarks::reset(n); }
};

struct StreamEntry {      // one per pushed stream; also read by the scatter / carry kernels
    uint32_t stream;      // slot index
    uint32_t len;         // samples of the new chunk
    uint32_t keep;        // carry length after this push
    uint32_t zero_fill;   // flush: zeros appended after the pending samples
    uint64_t src_off;     // offset of the chunk in the flat staging buffer (host pushes)
    uint64_t out_off;     // first float of the rows this push emits for the stream ([frame][n_mels], read by the VAD stage)
    uint32_t frames;      // rows emitted
    uint32_t act_base;    // index of the stream's first activity record of this push (records are packed in entry order)
};

// The admission of a push, entry by entry, for every bank's planner: the id is in range, a stream appears once per push, the chunk fits
// the slot; an admitted entry gets its place in the flat staging buffer and, with place(), the place of its rows.
struct PushAdmission {
    PushMarks &m;
    uint32_t n_streams, max_chunk, n_mels;
    uint64_t src_cursor = 0, out_cursor = 0;
    PushAdmission(PushMarks &marks, uint32_t n_streams_, uint32_t max_chunk_, uint32_t n_mels_) : m(marks), n_streams(n_streams_), max_chunk(max_chunk_), n_mels(n_mels_) {
        if (++m.epoch == 0) { std::fill(m.mark.begin(), m.mark.end(), 0u); m.epoch = 1; }
    }
    // 0 ok, 1 invalid argument, 2 capacity; *err names the problem
    int admit(uint32_t s, uint32_t len, StreamEntry &e, const char **err) {
        if (s >= n_streams) { *err = "stream id out of range"; return 1; }
        if (m.mark[s] == m.epoch) { *err = "a stream may appear only once per push"; return 1; }
        m.mark[s] = m.epoch;
        if (len > max_chunk) { *err = "chunk longer than max_chunk"; return 2; }
        e = StreamEntry{};
        e.stream = s; e.len = len; e.src_off = src_cursor;
        src_cursor += len;
        return 0;
    }
    // the entry emits `frames` rows: behind the rows of the entries before it
    void place(StreamEntry &e, uint64_t frames) {
        e.out_off = out_cursor; e.frames = static_cast<uint32_t>(frames);
        out_cursor += frames * n_mels;
    }
    uint64_t total_frames() const { return n_mels ? out_cursor / n_mels : 0; }
};

struct StreamPlan {
    std::vector<StreamEntry> entries;
    std::vector<uint64_t> off, len, out_off;   // ragged batch over the state buffer: sample offset / length, output offset
    std::vector<uint32_t> frames;
    uint64_t total_frames = 0;
};

// adds this push would make (h) and how many of the first ones return None (skip)
inline void stream_count(const StreamGeom &g, uint32_t pend, uint64_t idx, uint32_t len, bool flush, uint32_t &h, uint32_t &skip) {
    uint64_t idx_after_first;
    if (flush) {                         // add() with pcm_size < hop: zero-padded, idx += pcm_size (src/stft.rs:57-66)
        h = pend ? 1 : 0;
        idx_after_first = idx + pend;
    } else {
        h = (pend + len) / g.hop;
        idx_after_first = idx + g.hop;
    }
    skip = 0;                            // add j (0-based) emits iff idx_after_first + j*hop >= n_fft (src/stft.rs:68)
    if (idx_after_first < g.n_fft) {
        const uint64_t need = (g.n_fft - idx_after_first + g.hop - 1) / g.hop;
        skip = need < h ? static_cast<uint32_t>(need) : h;
    }
}

// returns 0 ok, 1 invalid argument, 2 capacity; *err names the problem
inline int stream_plan_push(const StreamGeom &g, StreamBook &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool flush,
                            StreamPlan &pl, const char **err) {
    pl.entries.resize(n); pl.off.resize(n); pl.len.resize(n); pl.out_off.resize(n); pl.frames.resize(n);
    PushAdmission adm(bk, g.n_streams, g.max_chunk, g.n_mels);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i], len = flush ? 0 : lens[i];
        StreamEntry &e = pl.entries[i];
        if (const int rc = adm.admit(s, len, e, err)) return rc;
        const uint32_t pend = bk.pending[s];
        const uint32_t c = g.n_fft - g.hop + pend;                   // current carry
        uint32_t h, skip;
        stream_count(g, pend, bk.idx[s], len, flush, h, skip);
        const uint32_t frames = h - skip;
        adm.place(e, frames);
        pl.frames[i] = frames;
        pl.off[i] = static_cast<uint64_t>(s) * g.stride + g.in_off - c + static_cast<uint64_t>(skip) * g.hop;
        pl.len[i] = frames ? static_cast<uint64_t>(frames - 1) * g.hop + g.n_fft : 0;
        pl.out_off[i] = e.out_off;
        e.zero_fill = flush && pend ? g.hop - pend : 0;
        e.keep = g.n_fft - g.hop + (flush ? 0 : pend + len - h * g.hop);
        e.act_base = static_cast<uint32_t>(g.n_mels ? e.out_off / g.n_mels : 0);
    }
    pl.total_frames = adm.total_frames();
    return 0;
}

inline void stream_commit_push(const StreamGeom &g, StreamBook &bk, const uint32_t *ids, const uint32_t *lens, uint32_t n, bool flush) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = ids[i];
        if (flush) { bk.idx[s] += bk.pending[s]; bk.pending[s] = 0; continue; }
        const uint32_t tot = bk.pending[s] + lens[i], h = tot / g.hop;
        bk.idx[s] += static_cast<uint64_t>(h) * g.hop;
        bk.pending[s] = tot - h * g.hop;
    }
}

inline size_t stream_frames_after(const StreamGeom &g, const StreamBook &bk, uint32_t id, uint32_t n_new) {
    uint32_t h, skip;
    stream_count(g, bk.pending[id], bk.idx[id], n_new, false, h, skip);
    return h - skip;
}

// ---- the push cache's key -----------------------------------------------------------------------------------------------------------
// Steady state of a live bank: the same streams pushing the same number of samples from the same pending count, every stream past its
// first window.  Such a push has the entry table and the ragged plan of the previous one, and both are still on the device (the bank
// keeps the pointers; this is the host side: what the push looked like).
struct PushQuery {                       // a push as the key sees it
    const uint32_t *ids = nullptr, *lens = nullptr;
    uint32_t n = 0;
    int fpu = 0;                         // frames per unit of the kernel the batch is planned for (AUTO may change its regime)
    int io = 0;                          // pcm | out << 4: the cached entries and plan count in elements of these types
    const void *d_out = nullptr;
    const uint64_t *h_out_off = nullptr; // the caller's row offsets (NULL: packed)
    const uint64_t *h_src_off = nullptr; // a device producer's chunk offsets (NULL: back to back -- they follow from lens)
    bool repeatable = true;              // mel rows of a push; not a flush, not an STFT emit
};

struct PushKey {
    bool valid = false;
    uint32_t n = 0;
    int fpu = 0, io = 0;
    const void *d_out = nullptr;
    std::vector<uint32_t> ids, lens, pend;
    std::vector<uint64_t> out_off, src_off;      // empty: the push had none

    void invalidate() { valid = false; }
    // does the push repeat the one the key was filled from?  (pending before the push; every stream was past its first window then and
    // idx only grows; a reset invalidates)
    bool matches(const StreamBook &bk, const PushQuery &q) const {
        if (!valid || !q.repeatable || n != q.n || d_out != q.d_out || fpu != q.fpu || io != q.io) return false;
        if (out_off.empty() != (q.h_out_off == nullptr) || src_off.empty() != (q.h_src_off == nullptr)) return false;
        for (uint32_t i = 0; i < n; ++i)
            if (q.ids[i] != ids[i] || q.lens[i] != lens[i] || bk.pending[q.ids[i]] != pend[i]) return false;
        const size_t bytes = static_cast<size_t>(n) * sizeof(uint64_t);
        return (!q.h_src_off || std::memcmp(q.h_src_off, src_off.data(), bytes) == 0) && (!q.h_out_off || std::memcmp(q.h_out_off, out_off.data(), bytes) == 0);
    }
    // before the push is committed.  A push that can come again: every stream past its first window (no skipped hops).  Returns valid.
    bool fill(const StreamGeom &g, const StreamBook &bk, const PushQuery &q) {
        valid = q.repeatable;
        for (uint32_t i = 0; i < q.n && valid; ++i) valid = bk.idx[q.ids[i]] >= g.n_fft;
        if (!valid) return false;
        n = q.n; fpu = q.fpu; io = q.io; d_out = q.d_out;
        ids.assign(q.ids, q.ids + n); lens.assign(q.lens, q.lens + n);
        pend.resize(n);
        for (uint32_t i = 0; i < n; ++i) pend[i] = bk.pending[ids[i]];
        if (q.h_out_off) out_off.assign(q.h_out_off, q.h_out_off + n); else out_off.clear();
        if (q.h_src_off) src_off.assign(q.h_src_off, q.h_src_off + n); else src_off.clear();
        return true;
    }
};

}  // namespace melspec
