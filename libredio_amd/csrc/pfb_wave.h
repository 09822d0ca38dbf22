// pfb_wave.h -- what the five 64-channel wave kernels of the polyphase banks share besides their lane programs (pfb_core.h): pfb64_kernel,
// pfbspec64_kernel, pfb_synth64_kernel, pfb_os64_kernel and pfb_os_synth64_kernel.  Device side: the twiddle prologue.  Host side: the
// taps / fused dispatch of the launchers that dispatch on nothing else (pfb64_kernel's and pfbspec64_kernel's also choose the input
// format, the layout and the cache policy, and keep their own).  The tile transform itself stays written out in every kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

namespace redio {

// The 64-point transform's twiddles, once per wavefront (pfb_core.h: why not inside the tile loop): declares twone = tw[0] and twa1 / twa2 /
// twa3[k2] = tw[4 k2], tw[8 k2], tw[12 k2] of passes A/B in 20 scalar registers, and the lane's twc1 / twc2 / twc3[k2] = tw[k], tw[2 k],
// tw[3 k] (k = k2 + 4 (lane & 3)) of pass C in 24 vector registers, kept where they are: no reload, no rematerialisation inside the loop.
// tw: the plan's forward or inverse table.  A macro, so that every kernel compiles to the instruction stream it had with these lines in
// its own body (profiles/r20_pfb_banks_resources.txt).
#define PFB_WAVE_TWIDDLES(tw, lane)                                                                                                              \
    float2 twone = (tw)[0], twa1[4], twa2[4], twa3[4], twc1[4], twc2[4], twc3[4];                                                                \
    _Pragma("unroll") for (int k2 = 0; k2 < 4; ++k2) {                                                                                           \
        twa1[k2] = (tw)[4 * k2]; twa2[k2] = (tw)[8 * k2]; twa3[k2] = (tw)[12 * k2];                                                              \
        const int k = k2 + 4 * ((lane) & 3);                                                                                                     \
        twc1[k2] = (tw)[k]; twc2[k2] = (tw)[2 * k]; twc3[k2] = (tw)[3 * k];                                                                      \
    }                                                                                                                                            \
    _Pragma("unroll") for (int k2 = 0; k2 < 4; ++k2) {                                                                                           \
        asm volatile("" : "+v"(twc1[k2].x), "+v"(twc1[k2].y), "+v"(twc2[k2].x), "+v"(twc2[k2].y), "+v"(twc3[k2].x), "+v"(twc3[k2].y));           \
        asm volatile("" : "+s"(twa1[k2].x), "+s"(twa1[k2].y), "+s"(twa2[k2].x), "+s"(twa2[k2].y), "+s"(twa3[k2].x), "+s"(twa3[k2].y));           \
    }                                                                                                                                            \
    asm volatile("" : "+s"(twone.x), "+s"(twone.y))

// go(std::integral_constant<int, P>, std::bool_constant<FUSED>) for the taps per branch the wave kernels are built for; any other P is
// hipErrorNotSupported.  16 first and fused first: the order in which the kernels have always been instantiated.
template <typename Go>
inline hipError_t pfb_wave_dispatch(int taps_per_branch, bool fused, Go &&go)
{
    switch (taps_per_branch) {
    case 16: return fused ? go(std::integral_constant<int, 16>{}, std::true_type{}) : go(std::integral_constant<int, 16>{}, std::false_type{});
    case 8: return fused ? go(std::integral_constant<int, 8>{}, std::true_type{}) : go(std::integral_constant<int, 8>{}, std::false_type{});
    case 4: return fused ? go(std::integral_constant<int, 4>{}, std::true_type{}) : go(std::integral_constant<int, 4>{}, std::false_type{});
    default: return hipErrorNotSupported;
    }
}

} // namespace redio
