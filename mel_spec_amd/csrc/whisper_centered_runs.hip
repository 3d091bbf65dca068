// whisper_centered_runs.hip -- the f32 six-frame run kernel of the centred Whisper features (whisper400_six_runs_raw_kernel,
// whisper_centered_kernels.hpp: MELSPEC_PRECISION_F32 on the 80-mel bank), as a translation unit of its own: it is compiled with
// melspec_runs.hip's scheduling strategy (mel_spec_amd/build.py), and the kernels of that unit keep the neighbours -- and so the
// instructions -- they have.
#include "whisper_centered_kernels.hpp"

namespace melspec {

template __global__ void whisper400_six_runs_raw_kernel<kSixMaxSlots, LensSix80>(const WcRawParams);

}  // namespace melspec
