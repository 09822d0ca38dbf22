// fft_ct_hi.hip -- the compile-time mixed-radix kernels (fft_ct.h) of the sizes 2160 ... 16200.
#include "fft_ct.h"

namespace redio {

#define REDIO_CT_INSTANCE(NN) template hipError_t launch_fft_ct<NN>(const FftPlanDev &, const float2 *, float2 *, long, long, bool, hipStream_t);
REDIO_FFT_CT_SIZES_HI(REDIO_CT_INSTANCE)
#undef REDIO_CT_INSTANCE

} // namespace redio
