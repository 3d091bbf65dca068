// fbank512_io.hip -- the NeMo / Parakeet frontend with int16 PCM in and / or f16 / bf16 rows out (fbank512_io_kernels.hpp): the f64 kernel
// (eight waves) and the f32 kernel (twelve waves, staged rows) of the compile-time 80- and 128-mel Slaney banks, and the normalisers that
// read f32 rows and write 16-bit ones.  Kept out of fbank512.hip so that its kernels stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_io_kernels.hpp"

namespace melspec {

#define MS_IO_INST(In, Out)                                                                                                   \
    template __global__ void fbank512_nemo_io_kernel<double, 8, kBlmSlots, LensSlaney128, In, Out>(const FbankFastParams);  \
    template __global__ void fbank512_nemo_io_kernel<double, 8, kFbSlots, LensSlaney80, In, Out>(const FbankFastParams);    \
    template __global__ void fbank512_nemo_io_kernel<float, 12, kBlmSlots, LensSlaney128, In, Out>(const FbankFastParams);  \
    template __global__ void fbank512_nemo_io_kernel<float, 12, kFbSlots, LensSlaney80, In, Out>(const FbankFastParams);
MS_IO_COMBOS(MS_IO_INST)
#undef MS_IO_INST

template __global__ void blm_normalize_io_kernel<io_f16>(const BlmNormIoParams);
template __global__ void blm_normalize_io_kernel<io_bf16>(const BlmNormIoParams);
template __global__ void blm_normalize_ragged_io_kernel<io_f16>(const BlmNormRaggedIoParams);
template __global__ void blm_normalize_ragged_io_kernel<io_bf16>(const BlmNormRaggedIoParams);

}  // namespace melspec
