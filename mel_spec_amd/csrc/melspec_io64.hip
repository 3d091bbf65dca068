// melspec_io64.hip -- the f64 six-frame kernel with int16 PCM in and / or f16 / bf16 rows out (whisper400_io_kernels.hpp): the 80- and
// 128-mel Whisper banks in MELSPEC_PRECISION_F64 and AUTO's gated second launch.  Default scheduling strategy, like whisper400.hip, where
// the f32-in / f32-out originals live; a unit of its own so that those stay the instructions they are.
#include "whisper400_io_kernels.hpp"

namespace melspec {

#define MS_IO_INST(In, Out)                                                                                   \
    template __global__ void whisper400_six64_io_kernel<kSixMaxSlots, LensSix80, In, Out>(const Six64Params); \
    template __global__ void whisper400_six64_io_kernel<kSixWideSlots, LensSix128, In, Out>(const Six64Params);
MS_IO_COMBOS(MS_IO_INST)
#undef MS_IO_INST

}  // namespace melspec
