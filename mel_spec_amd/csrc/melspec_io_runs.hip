// melspec_io_runs.hip -- the run-per-wave f32 six-frame kernels with int16 PCM in and / or f16 / bf16 rows out (whisper400_io_kernels.hpp):
// the 80- and 128-mel Whisper banks, compiled like their f32-in / f32-out originals in melspec_runs.hip (same scheduling strategy,
// mel_spec_amd/build.py) and kept out of that unit so that its kernels stay the instructions they are.
#include "whisper400_io_kernels.hpp"

namespace melspec {

#define MS_IO_INST(In, Out)                                                                                            \
    template __global__ void whisper400_six_runs_io_kernel<kSixMaxSlots, LensSix80, In, Out>(const FastParams);       \
    template __global__ void whisper400_six_wide_runs_io_kernel<kSixWideSlots, LensSix128, In, Out>(const FastParams);
MS_IO_COMBOS(MS_IO_INST)
#undef MS_IO_INST

}  // namespace melspec
