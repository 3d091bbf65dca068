// whisper_centered_io_runs.hip -- the f32 six-frame run kernel of the centred Whisper features with int16 PCM in / f16, bf16 rows out
// (whisper400_six_runs_raw_io_kernel, whisper_centered_io_kernels.hpp: MELSPEC_PRECISION_F32 on the 80-mel bank), as a translation unit of
// its own with whisper_centered_runs.hip's scheduling strategy (mel_spec_amd/build.py): the kernels of that unit keep the neighbours -- and
// so the instructions -- they have.
#include "whisper_centered_io_kernels.hpp"

namespace melspec {

#define MS_IO_INST(In, Out) MS_WC_IO_RUNS(template __global__ void, In, Out)
MS_IO_COMBOS(MS_IO_INST)
#undef MS_IO_INST

}  // namespace melspec
