// stat_bank_tail.hpp -- the table that travels behind a push's entries (stream_bank.hpp: core_run's tail) for the Kaldi fbank's and the
// NeMo / Parakeet frontend's stream banks (plain C++, no HIP).  Shared by stat_bank.hpp, fbank512.hip and tests/cpp/stat_bank_tail_host.cpp.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace melspec {

// the Kaldi bank's own table: the clips' continues flags, u32[n]
inline std::vector<unsigned char> fbank_stream_own_tail(const uint32_t *continues, uint32_t n) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(continues);
    return std::vector<unsigned char>(p, p + static_cast<size_t>(n) * sizeof(uint32_t));
}

// the NeMo bank's own table: the clips' sample counts, u64[n], and behind them their window origins, i32[n]
inline size_t blm_stream_org0_at(uint32_t n) { return static_cast<size_t>(n) * sizeof(uint64_t); }
inline std::vector<unsigned char> blm_stream_own_tail(const uint64_t *len, const int32_t *org0, uint32_t n) {
    std::vector<unsigned char> own(blm_stream_org0_at(n) + static_cast<size_t>(n) * sizeof(int32_t));
    std::memcpy(own.data(), len, blm_stream_org0_at(n));
    std::memcpy(own.data() + blm_stream_org0_at(n), org0, static_cast<size_t>(n) * sizeof(int32_t));
    return own;
}

// What a push sends.  An f32 push: the bank's own table as it is.  A push with 16-bit rows (stream_banks_io_kernels.hpp): the fold behind
// the frame stage needs each entry's place in the bank's f32 scratch beside its place in the caller's rows (the entries' out_off), so the
// plan's packed offsets follow the bank's table, 8-byte aligned.
struct TypedTail {
    std::vector<unsigned char> joined;
    const void *data;
    size_t bytes, packed_at = 0;
    TypedTail(const void *own, size_t own_bytes, const uint64_t *packed_off, uint32_t n) : data(own), bytes(own_bytes) {
        if (!packed_off) return;
        packed_at = (own_bytes + 7) & ~static_cast<size_t>(7);
        joined.resize(packed_at + static_cast<size_t>(n) * sizeof(uint64_t));
        std::memcpy(joined.data(), own, own_bytes);
        std::memcpy(joined.data() + packed_at, packed_off, static_cast<size_t>(n) * sizeof(uint64_t));
        data = joined.data(); bytes = joined.size();
    }
    const uint64_t *packed_on_device(const void *d_tail) const { return reinterpret_cast<const uint64_t *>(static_cast<const char *>(d_tail) + packed_at); }
};

}  // namespace melspec
