// The table behind a push's entries of the Kaldi and the NeMo / Parakeet stream bank (mel_spec_amd/csrc/stat_bank_tail.hpp), on the host:
// the bank's own table -- Kaldi: continues u32[n]; NeMo: len u64[n], then org0 i32[n] at byte n * 8 -- and TypedTail, which sends it as it is
// for an f32 push and with the plan's packed offsets behind it, 8-byte aligned, for a push with 16-bit rows.  The "device" is a copy of
// what TypedTail hands to core_run, at an 8-byte aligned address as a ring slot's is.
// Links nothing but the header.  Prints "stat_bank_tail_host: ok"; exit status 1 on any mismatch.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "stat_bank_tail.hpp"

using namespace melspec;

static int g_failures = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            if (g_failures++ < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                                                    \
    } while (0)

static void check_tail(const char *who, uint32_t n, const std::vector<unsigned char> &own, size_t want_own_bytes, size_t want_packed_at) {
    CHECK(own.size() == want_own_bytes, "%s n %u: own table of %zu bytes, want %zu", who, n, own.size(), want_own_bytes);
    std::vector<uint64_t> packed(n);
    for (uint32_t i = 0; i < n; ++i) packed[i] = 0x0123456789abcdefull * (i + 1) + n;

    // an f32 push: the own table itself, nothing copied
    const TypedTail plain(own.data(), own.size(), nullptr, n);
    CHECK(plain.data == own.data() && plain.bytes == own.size() && plain.joined.empty() && plain.packed_at == 0, "%s n %u: an f32 push copied its table", who, n);

    // 16-bit rows: own bytes verbatim, then the packed offsets at the own size rounded up to 8
    const TypedTail typed(own.data(), own.size(), packed.data(), n);
    CHECK(typed.packed_at == want_packed_at && typed.packed_at % 8 == 0 && typed.packed_at >= own.size() && typed.packed_at < own.size() + 8,
          "%s n %u: packed_at %zu, want %zu", who, n, typed.packed_at, want_packed_at);
    CHECK(typed.data == typed.joined.data() && typed.bytes == typed.joined.size() && typed.bytes == want_packed_at + n * sizeof(uint64_t),
          "%s n %u: joined table of %zu bytes", who, n, typed.bytes);
    CHECK(typed.bytes >= own.size() && std::memcmp(typed.data, own.data(), own.size()) == 0, "%s n %u: the own bytes changed on the way", who, n);
    std::vector<uint64_t> device((typed.bytes + 7) / 8 + 1, ~0ull);
    std::memcpy(device.data(), typed.data, typed.bytes);
    const uint64_t *d_packed = typed.packed_on_device(device.data());
    CHECK(reinterpret_cast<const unsigned char *>(d_packed) + n * sizeof(uint64_t) <= reinterpret_cast<const unsigned char *>(device.data()) + typed.bytes,
          "%s n %u: the packed offsets end behind the table", who, n);
    for (uint32_t i = 0; i < n; ++i) CHECK(d_packed[i] == packed[i], "%s n %u: packed offset %u reads %llx", who, n, i, static_cast<unsigned long long>(d_packed[i]));
}

int main() {
    for (uint32_t n : {1u, 2u, 3u, 5u, 8u}) {
        std::vector<uint32_t> cont(n);
        std::vector<uint64_t> len(n);
        std::vector<int32_t> org0(n);
        for (uint32_t i = 0; i < n; ++i) {
            cont[i] = (i * 7 + n) % 2;
            len[i] = 0x100000000ull * (i + 1) + 400 + i;       // both halves of the word are told apart
            org0[i] = static_cast<int32_t>(i) * 57 - 200;
        }
        const std::vector<unsigned char> kaldi = fbank_stream_own_tail(cont.data(), n);
        CHECK(kaldi.size() == n * 4 && std::memcmp(kaldi.data(), cont.data(), n * 4) == 0, "kaldi n %u: the table is not the continues flags", n);
        check_tail("kaldi", n, kaldi, n * 4, (n * 4 + 7) / 8 * 8);

        const std::vector<unsigned char> nemo = blm_stream_own_tail(len.data(), org0.data(), n);
        CHECK(blm_stream_org0_at(n) == n * 8, "nemo n %u: org0 at byte %zu", n, blm_stream_org0_at(n));
        CHECK(nemo.size() == n * 12 && std::memcmp(nemo.data(), len.data(), n * 8) == 0 && std::memcmp(nemo.data() + n * 8, org0.data(), n * 4) == 0,
              "nemo n %u: the table is not len, then org0", n);
        check_tail("nemo", n, nemo, n * 12, (n * 12 + 7) / 8 * 8);
    }
    // the sizes written out
    uint32_t c1 = 1;
    uint64_t l3[3] = {1, 2, 3};
    int32_t o3[3] = {-200, 56, 0};
    uint64_t p3[3] = {0, 80, 160};
    const std::vector<unsigned char> k1 = fbank_stream_own_tail(&c1, 1), n1 = blm_stream_own_tail(l3, o3, 1), n3 = blm_stream_own_tail(l3, o3, 3);
    CHECK(TypedTail(k1.data(), k1.size(), p3, 1).packed_at == 8, "kaldi n 1: 4 -> 8");
    CHECK(TypedTail(n1.data(), n1.size(), p3, 1).packed_at == 16, "nemo n 1: 12 -> 16");
    CHECK(TypedTail(n3.data(), n3.size(), p3, 3).packed_at == 40, "nemo n 3: 36 -> 40");
    if (g_failures) { std::printf("stat_bank_tail_host: %d failures\n", g_failures); return 1; }
    std::printf("stat_bank_tail_host: ok\n");
    return 0;
}
