// fbank512_kaldi_io.hip -- the Kaldi fbank with int16 PCM in and / or f16 / bf16 rows out (fbank512_kaldi_io_kernels.hpp): the wave-owned
// f64 kernel (eight waves, a run of units per wave) of the compile-time 80-bin Kaldi bank, and the CMN that reads f32 rows and writes
// 16-bit ones.  Kept out of fbank512.hip and fbank512_io.hip so that their kernels stay the instructions they are.
#define MS_FBANK512_NO_PLAIN_KERNELS       // blm_normalize_kernel / blm_normalize_ragged_kernel live in fbank512.hip
#include "fbank512_kaldi_io_kernels.hpp"

namespace melspec {

#define MS_IO_INST(In, Out) template __global__ void fbank512_kaldi_io_kernel<double, 8, kFbSlots, LensKaldi80, In, Out>(const FbankFastParams);
MS_IO_COMBOS(MS_IO_INST)
#undef MS_IO_INST

template __global__ void cmn_io_kernel<io_f16>(const CmnIoParams);
template __global__ void cmn_io_kernel<io_bf16>(const CmnIoParams);

}  // namespace melspec
