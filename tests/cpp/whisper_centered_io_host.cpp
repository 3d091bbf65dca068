// whisper_centered_io_host.cpp -- the arithmetic the 16-bit ends of the centred Whisper features add to the host side
// (mel_spec_amd/csrc/whisper_centered_plan.hpp: melspec_whisper_*_io): the element sizes of the dtype codes, the alignment rule of the
// device pointers, the order of the argument verdicts with the dtype codes in front, and the 16-byte store rule of the finalise pass
// against the addresses it stands for, address by address.  Stand-alone, no HIP, never loaded into Python, never on a GPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Imel_spec_amd/csrc tests/cpp/whisper_centered_io_host.cpp -o /tmp/whisper_centered_io_host && /tmp/whisper_centered_io_host
#include <cstdio>
#include <cstring>

#include "whisper_centered_plan.hpp"

using namespace melspec::host;

static int bad = 0;
#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            if (++bad <= 20) { std::printf("FAILED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                  \
    } while (0)

int main() {
    // ---- the dtype codes ----
    CHECK(wc_pcm_known(MELSPEC_PCM_F32) && wc_pcm_known(MELSPEC_PCM_S16) && !wc_pcm_known(2) && !wc_pcm_known(-1), "pcm codes");
    CHECK(wc_out_known(MELSPEC_OUT_F32) && wc_out_known(MELSPEC_OUT_F16) && wc_out_known(MELSPEC_OUT_BF16) && !wc_out_known(3) && !wc_out_known(-1), "out codes");
    CHECK(wc_pcm_bytes(MELSPEC_PCM_F32) == 4 && wc_pcm_bytes(MELSPEC_PCM_S16) == 2, "sample sizes");
    CHECK(wc_out_bytes(MELSPEC_OUT_F32) == 4 && wc_out_bytes(MELSPEC_OUT_F16) == 2 && wc_out_bytes(MELSPEC_OUT_BF16) == 2, "output sizes");

    // ---- natural alignment, nothing more ----
    alignas(16) static char mem[64];
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b)
            for (int pcm = 0; pcm < 2; ++pcm)
                for (int out = 0; out < 3; ++out) {
                    const bool want = a % (pcm ? 2 : 4) != 0 || b % (out ? 2 : 4) != 0;
                    CHECK(wc_io_misaligned(mem + a, pcm, mem + 32 + b, out) == want, "bytes %d / %d, (%d, %d)", a, b, pcm, out);
                }

    // ---- the verdicts: ctx, dtype codes, then wc_args's order, the alignment with the device pointers ----
    const uint64_t tab[1] = {0};
    auto v = [&](bool ctx, bool sup, int pcm, int out, uint64_t pad, uint32_t n, uint64_t total, const void *p, const void *r, bool split, const void *mx) {
        return wc_args_io(ctx, sup, pcm, out, pad, true, n, tab, tab, 0, 0, total, p, r, split, mx);
    };
    const void *even = mem, *odd = mem + 1, *two = mem + 2;
    {
        WcArgs a = v(false, false, 7, 7, 1, 1, 1, nullptr, nullptr, false, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && std::strstr(a.msg, "ctx"), "NULL context first");
        a = v(true, false, 2, 0, 1, 1, 1, nullptr, nullptr, false, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && std::strstr(a.msg, "pcm_dtype"), "unknown pcm code before the support check");
        a = v(true, false, 1, 3, 1, 1, 1, nullptr, nullptr, false, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && std::strstr(a.msg, "out_dtype"), "unknown out code before the support check");
        a = v(true, false, 1, 1, 1, 1, 1, odd, odd, false, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_UNSUPPORTED && a.msg == nullptr, "unsupported before pad_to and the pointers");
        a = v(true, true, 1, 1, 399, 1, 1, odd, odd, false, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && std::strstr(a.msg, "pad_to"), "pad_to before the pointers");
        a = v(true, true, 1, 1, 0, 0, 0, odd, odd, false, nullptr);
        CHECK(a.verdict == kWcDone, "no clips: done, whatever the pointers");
        a = v(true, true, 1, 1, 0, 1, 0, odd, odd, true, even);
        CHECK(a.verdict == kWcSlots, "no frame, split: the maxima alone, the pointers are not looked at");
        a = v(true, true, 1, 1, 0, 1, 1, nullptr, even, false, nullptr);
        CHECK(a.verdict == kWcFail && std::strstr(a.msg, "NULL"), "NULL device pointer");
        a = v(true, true, 1, 1, 0, 1, 1, odd, even, false, nullptr);
        CHECK(a.verdict == kWcFail && a.status == MELSPEC_ERR_INVALID_ARG && std::strstr(a.msg, "aligned"), "odd byte address, int16 PCM");
        a = v(true, true, 1, 2, 0, 1, 1, even, odd, true, even);
        CHECK(a.verdict == kWcFail && std::strstr(a.msg, "aligned"), "odd byte address, bf16 rows");
        a = v(true, true, 1, 0, 0, 1, 1, two, two, false, nullptr);
        CHECK(a.verdict == kWcFail && std::strstr(a.msg, "aligned"), "f32 output at a 2-byte address");
        a = v(true, true, 1, 1, 0, 1, 1, two, two, false, nullptr);
        CHECK(a.verdict == kWcGo, "2-byte addresses are enough for (S16, F16)");
        a = v(true, true, 1, 1, 0, 1, 1, two, two, true, nullptr);
        CHECK(a.verdict == kWcFail && std::strstr(a.msg, "d_clip_max"), "d_clip_max");
        // (F32, F32) is wc_args itself: the f32 calls never looked at the alignment
        a = v(true, true, 0, 0, 0, 1, 1, odd, odd, false, nullptr);
        const WcArgs b = wc_args(true, true, 0, true, 1, tab, tab, 0, 0, 1, odd, odd, false, nullptr);
        CHECK(a.verdict == b.verdict && a.status == b.status && a.verdict == kWcGo, "(F32, F32)");
    }

    // ---- the 16-byte store rule: when it holds, every piece of every full tile of every mel row starts at a 16-byte address ----
    for (size_t es : {size_t(2), size_t(4)}) {
        const uint64_t vec = 16 / es;
        for (uint64_t T = 60; T <= 140; ++T)
            for (uint64_t off = 0; off < 20; ++off)
                for (uintptr_t base = 4096; base < 4096 + 32; base += es) {
                    const bool ok = wc_wide_ok(T, off, base, es);
                    bool all = true;          // by the addresses: piece q of row m of tile k
                    for (uint64_t m = 0; m < 3 && all; ++m)
                        for (uint64_t k = 0; (k + 1) * 64 <= T && all; ++k)
                            for (uint64_t q = 0; q < 64 / vec; ++q)
                                if ((base + (off + m * T + 64 * k + vec * q) * es) % 16 != 0) { all = false; break; }
                    // the rule may be stricter than the addresses (it does not look at a single row), never laxer
                    CHECK(!ok || all, "es %zu T %llu off %llu base %llu: wide, but a piece is not 16-byte aligned", es, (unsigned long long)T, (unsigned long long)off,
                          (unsigned long long)base);
                    CHECK(ok == ((T % vec == 0) && (off % vec == 0) && (base % 16 == 0)), "es %zu T %llu off %llu base %llu", es, (unsigned long long)T,
                          (unsigned long long)off, (unsigned long long)base);
                }
    }
    // the tests' landmarks: T = 68 is wide for f32 alone, 72 and 136 for both; WHISPER's 3000-frame clips always qualify, packed
    CHECK(wc_wide_ok(68, 0, 4096, 4) && !wc_wide_ok(68, 0, 4096, 2) && wc_wide_ok(72, 0, 4096, 2) && wc_wide_ok(136, 8, 4096, 2), "68 / 72 / 136");
    for (uint64_t clip = 0; clip < 4; ++clip)
        for (int nm : {80, 128}) CHECK(wc_wide_ok(3000, clip * 3000 * nm, 4096, 2) && wc_wide_ok(3000, clip * 3000 * nm, 4096, 4), "3000 frames");
    CHECK(!wc_wide_ok(64, 1, 4096, 2) && !wc_wide_ok(64, 4, 4096, 2) && wc_wide_ok(64, 4, 4096, 4) && !wc_wide_ok(64, 0, 4098, 2), "offsets and bases");

    if (bad) { std::printf("whisper_centered_io_host: %d checks FAILED\n", bad); return 1; }
    std::printf("whisper_centered_io_host: ok\n");
    return 0;
}
