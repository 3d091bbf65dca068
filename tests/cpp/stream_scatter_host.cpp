// stream_scatter_host.cpp -- the index arithmetic of the typed stream_scatter_kernel (mel_spec_amd/csrc/aux_kernels.hpp) on the host,
// for a sanitizer: the plan is the bank's own (stream_plan.hpp), the staging buffer and the state are heap blocks of exactly the sizes
// the bank allocates (csrc/stream_bank.hpp: core_create, core_push_host) less their slack, and the loop below restates the kernel -- a block per entry, 256 lanes striding the chunk,
// source at src_off + i in ELEMENTS of the sample type, value int16 * 2^-15.  A read or write outside either block is an ASan report;
// the state is compared with the same pushes of the converted f32 chunks.  Stand-alone, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/stream_scatter_host.cpp -o /tmp/stream_scatter_host && /tmp/stream_scatter_host
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "stream_plan.hpp"

using namespace melspec;

static float sample(float v) { return v; }
static float sample(int16_t v) { return static_cast<float>(v) * 0x1p-15f; }

template <class S>
static void scatter(float *state, uint64_t stride, uint32_t in_off, const StreamEntry *entries, uint32_t n, const S *src) {
    for (uint32_t block = 0; block < n; ++block)
        for (uint32_t tid = 0; tid < 256; ++tid) {
            const StreamEntry e = entries[block];
            float *dst = state + e.stream * stride + in_off;
            if (src)
                for (uint32_t i = tid; i < e.len; i += 256) dst[i] = sample(src[e.src_off + i]);
            for (uint32_t i = tid; i < e.zero_fill; i += 256) dst[e.len + i] = 0.0f;
        }
}

static void carry(float *state, uint64_t stride, uint32_t in_off, const StreamEntry *entries, uint32_t n) {
    for (uint32_t b = 0; b < n; ++b) {
        const StreamEntry e = entries[b];
        const uint32_t m = e.len + e.zero_fill;
        if (m == 0) continue;
        float *slot = state + e.stream * stride;
        std::memmove(slot + in_off - e.keep, slot + in_off + m - e.keep, e.keep * sizeof(float));
    }
}

int main() {
    const uint32_t n_streams = 5, max_chunk = 1000;
    const uint32_t sizes[] = {0, 1, 159, 160, 161, 320, 399, 400, 401, 1000};
    int bad = 0;
    for (uint32_t geo = 0; geo < 3; ++geo) {
        const uint32_t fft = geo == 0 ? 400 : geo == 1 ? 512 : 1024, hop = geo == 2 ? 256 : 160;
        const StreamGeom g = stream_geometry(fft, hop, 80, n_streams, max_chunk);
        StreamBook book16, book32;
        book16.reset(n_streams); book32.reset(n_streams);
        const size_t words = static_cast<size_t>(n_streams) * g.stride;
        std::unique_ptr<float[]> st16(new float[words]()), st32(new float[words]());
        std::mt19937 rng(17 + geo);
        for (int push = 0; push < 200; ++push) {
            const bool flush = push % 50 == 49;
            std::vector<uint32_t> ids, lens;
            for (uint32_t s = 0; s < n_streams; ++s)
                if (rng() % 10 < 7) {
                    ids.push_back(s);
                    lens.push_back(rng() & 1 ? sizes[rng() % 10] : rng() % (max_chunk + 1));
                }
            if (ids.empty()) continue;
            const uint32_t n = static_cast<uint32_t>(ids.size());
            StreamPlan p16, p32;
            const char *err = nullptr;
            if (stream_plan_push(g, book16, ids.data(), lens.data(), n, flush, p16, &err) || stream_plan_push(g, book32, ids.data(), lens.data(), n, flush, p32, &err)) {
                std::printf("plan failed: %s\n", err);
                return 2;
            }
            uint64_t total = 0;
            for (const StreamEntry &e : p16.entries) total += e.len;
            // exactly `total` elements each: the first element past a chunk that the loop touched would be outside the block
            std::unique_ptr<int16_t[]> src16(new int16_t[total]);
            std::unique_ptr<float[]> src32(new float[total]);
            for (uint64_t i = 0; i < total; ++i) {
                src16[i] = static_cast<int16_t>(rng());
                src32[i] = static_cast<float>(src16[i]) / 32768.0f;          // the reference's spelling of the conversion
            }
            scatter<int16_t>(st16.get(), g.stride, g.in_off, p16.entries.data(), n, total ? src16.get() : nullptr);
            scatter<float>(st32.get(), g.stride, g.in_off, p32.entries.data(), n, total ? src32.get() : nullptr);
            carry(st16.get(), g.stride, g.in_off, p16.entries.data(), n);
            carry(st32.get(), g.stride, g.in_off, p32.entries.data(), n);
            stream_commit_push(g, book16, ids.data(), lens.data(), n, flush);
            stream_commit_push(g, book32, ids.data(), lens.data(), n, flush);
            // what later frames read: every stream's carry, right-aligned at in_off
            for (uint32_t s = 0; s < n_streams; ++s) {
                const uint32_t keep = fft - hop + book16.pending[s];
                const size_t at = s * g.stride + g.in_off - keep;
                if (std::memcmp(st16.get() + at, st32.get() + at, keep * sizeof(float)) != 0) {
                    std::printf("geometry %u push %d stream %u: the int16 bank's carry differs from the f32 bank's\n", geo, push, s);
                    ++bad;
                }
            }
        }
    }
    std::printf(bad ? "FAILED\n" : "stream_scatter_host: ok\n");
    return bad ? 1 : 0;
}
