// whisper400_io_kernels.hpp -- the six-frame kernels of plain batches with the sample type (float, int16_t) and the row type (float, f16,
// bf16) as template parameters: melspec_compute_*_device_io / melspec_compute_host_io.  The bodies are those of whisper400_six_runs_kernel,
// whisper400_six_wide_runs_kernel and whisper400_six64_kernel (the same text, included again): same grid, same run per wave, same vote sample,
// same arithmetic; only the load of phase 1 / fix_load_samples (load2_unaligned's int16_t form: one 4-byte load per sample pair, times
// 2^-15, exact) and the store of phase 4 (one 16-bit store per lane and value, the f32 value rounded to nearest even) differ.  Instantiated
// in translation units of their own (melspec_io_runs.hip, melspec_io64.hip): a new neighbour in a unit changes the schedule of the kernels
// that are already there (melspec_runs.hip).
#pragma once
#include "whisper400_kernels.hpp"
#include "io_types.hpp"

namespace melspec {

template <int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(kSixWaves * 64, 4) void whisper400_six_runs_io_kernel(const FastParams p) {
#define MS_SIX_RUNS_WAVES kSixWaves
#define MS_SIX_RUNS_IN In
#define MS_SIX_RUNS_OUT Out
#include "whisper400_six_runs_body.inc"
#undef MS_SIX_RUNS_OUT
#undef MS_SIX_RUNS_IN
#undef MS_SIX_RUNS_WAVES
}

template <int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(kSixWideWaves * 64, 3) void whisper400_six_wide_runs_io_kernel(const FastParams p) {
#define MS_SIX_RUNS_WAVES kSixWideWaves
#define MS_SIX_RUNS_IN In
#define MS_SIX_RUNS_OUT Out
#include "whisper400_six_runs_body.inc"
#undef MS_SIX_RUNS_OUT
#undef MS_SIX_RUNS_IN
#undef MS_SIX_RUNS_WAVES
}

template <int NSLOTS, class Lens, class In, class Out>
__global__ __launch_bounds__(kSix64Waves * 64, 3) void whisper400_six64_io_kernel(const Six64Params p) {
#define MS_SIX64_IN In
#define MS_SIX64_OUT Out
#include "whisper400_six64_body.inc"
#undef MS_SIX64_OUT
#undef MS_SIX64_IN
}

}  // namespace melspec
