// whisper_centered_io.hip -- the kernels of the centred Whisper features with int16 PCM in / f16, bf16 out that take the default scheduling
// strategy: the f64 raw kernels (whisper400_six64_raw_io_kernel, whisper_centered_io_kernels.hpp) and the typed forms of the small kernels
// (wc_prepare_kernel over the sample type, wc_fill_kernel / wc_finalize_kernel over the output type: whisper_centered_kernels.hpp).  A unit
// of its own so that the kernels of whisper_centered.hip keep the instructions they have; whisper_centered.hip launches these.
#include "whisper_centered_io_kernels.hpp"

namespace melspec {

#define MS_IO_INST(In, Out) MS_WC_IO_64(template __global__ void, In, Out)
MS_IO_COMBOS(MS_IO_INST)
#undef MS_IO_INST
MS_WC_IO_SMALL(template __global__ void)

}  // namespace melspec
