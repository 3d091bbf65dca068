// whisper_centered_io_kernels.hpp -- the raw six-frame kernels of the centred Whisper features with the sample type (float, int16_t) and
// the row type (float, f16, bf16) as template parameters: melspec_whisper_*_io.  The bodies are those of whisper400_six_runs_raw_kernel and
// whisper400_six64_raw_kernel (the same text, included again with MS_SIX_RUNS_RAW / MS_SIX64_RAW): same grid, same run per wave, same
// arithmetic, the same maximum folded from the f32 bits; only the load of phase 1 (load2_unaligned's int16_t form: sample * 2^-15, exact) and
// six_raw_store's store (one 16-bit store per lane and value, the f32 value rounded to nearest even) differ.  Instantiated in translation
// units of their own (whisper_centered_io_runs.hip, whisper_centered_io.hip), as whisper400_io_kernels.hpp's are: a new neighbour in a unit
// changes the schedule of the kernels that are already there.
#pragma once
#include "whisper_centered_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

template <int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(kSixWaves * 64, 4) void whisper400_six_runs_raw_io_kernel(const WcRawParams q) {
    const FastParams &p = q.f;
    int *const wc_slots = q.slots;
    const uint32_t *const wc_slot_map = q.slot_map;
#define MS_SIX_RUNS_RAW 1
#define MS_SIX_RUNS_WAVES kSixWaves
#define MS_SIX_RUNS_IN In
#define MS_SIX_RUNS_OUT Out
#include "whisper400_six_runs_body.inc"
#undef MS_SIX_RUNS_OUT
#undef MS_SIX_RUNS_IN
#undef MS_SIX_RUNS_WAVES
#undef MS_SIX_RUNS_RAW
}

template <int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(kSix64Waves * 64, 3) void whisper400_six64_raw_io_kernel(const WcRaw64Params q) {
    const Six64Params &p = q.f;
    int *const wc_slots = q.slots;
    const uint32_t *const wc_slot_map = q.slot_map;
#define MS_SIX64_RAW 1
#define MS_SIX64_IN In
#define MS_SIX64_OUT Out
#include "whisper400_six64_body.inc"
#undef MS_SIX64_OUT
#undef MS_SIX64_IN
#undef MS_SIX64_RAW
}

// the five (sample, row) combinations of the split calls; the normalised calls use (io_s16, float) alone (their raw rows stay f32), and the
// edge launch -- it reads the gathered f32 samples -- the (float, Out) ones
#define MS_WC_IO_RUNS(X, In, Out) X whisper400_six_runs_raw_io_kernel<kSixMaxSlots, LensSix80, In, Out>(const WcRawParams);
#define MS_WC_IO_64(X, In, Out)                                                                  \
    X whisper400_six64_raw_io_kernel<kSixMaxSlots, LensSix80, In, Out>(const WcRaw64Params);     \
    X whisper400_six64_raw_io_kernel<kSixWideSlots, LensSix128, In, Out>(const WcRaw64Params);
// the small kernels beside their float forms (whisper_centered.hip)
#define MS_WC_IO_SMALL(X)                                                                                                          \
    X wc_prepare_kernel<io_s16>(const io_s16 *, const host::WcEdge *, uint32_t, float *, int *, uint32_t);                         \
    X wc_fill_kernel<io_f16>(const host::WcRecord *, io_f16 *, int);                                                               \
    X wc_fill_kernel<io_bf16>(const host::WcRecord *, io_bf16 *, int);                                                             \
    X wc_finalize_kernel<io_f16>(const host::WcRecord *, const float *, const int *, io_f16 *, int, int);                          \
    X wc_finalize_kernel<io_bf16>(const host::WcRecord *, const float *, const int *, io_bf16 *, int, int);

}  // namespace melspec
