// fft_ct_lo.hip -- the compile-time mixed-radix kernels (fft_ct.h) of the sizes 6 ... 2025.
#include "fft_ct.h"

namespace redio {

#define REDIO_CT_INSTANCE(NN) template hipError_t launch_fft_ct<NN>(const FftPlanDev &, const float2 *, float2 *, long, long, bool, hipStream_t);
REDIO_FFT_CT_SIZES_LO(REDIO_CT_INSTANCE)
#undef REDIO_CT_INSTANCE

} // namespace redio
