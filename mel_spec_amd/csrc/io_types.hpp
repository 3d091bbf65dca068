// io_types.hpp -- the sample and row types of the *_io entry points (MELSPEC_PCM_*, MELSPEC_OUT_*) as the kernels name them.
#pragma once
#include <cstdint>

namespace melspec {

using io_s16 = int16_t;       // MELSPEC_PCM_S16
using io_f16 = _Float16;      // MELSPEC_OUT_F16: v_cvt_f16_f32, round to nearest even
using io_bf16 = __bf16;       // MELSPEC_OUT_BF16: v_cvt_pk_bf16_f32, round to nearest even, a NaN stays a NaN

// the five (sample, row) combinations beside (float, float), which is the existing kernels'
#define MS_IO_COMBOS(X) X(io_s16, float) X(float, io_f16) X(float, io_bf16) X(io_s16, io_f16) X(io_s16, io_bf16)

}  // namespace melspec
