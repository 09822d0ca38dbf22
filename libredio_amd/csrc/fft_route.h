// fft_route.h -- which kernel family a complex transform of nfft points takes: ONE decision, made from the size and its stage list
// alone, that the dispatcher (fft_kernels.hip: launch_fft), the C-ABI layer's staging (redio_api.hip) and every plan that owns a
// redio_fft (redio_fft_stages, redio_internal.h) share.  The order of the tests below is the specification: the sizes with a kernel
// of their own first, then the compile-time list, then the LDS kernels, then the global-memory families.
//
// No HIP type: tests/emu_route compiles it with g++ (tests/test_fft_route.py holds the expected table).
#pragma once

namespace redio {
#pragma GCC visibility push(hidden) // library-internal: nothing here joins the exported symbol set

// every 2^a 3^b 5^c size with a compile-time pass list (fft_ct.h), in two halves: one translation unit each (fft_ct_lo.hip,
// fft_ct_hi.hip).  The route's membership test and the dispatcher's switch expand the same list.
#define REDIO_FFT_CT_SIZES_LO(X)                                                                                         \
    X(6) X(9) X(10) X(12) X(15) X(18) X(20) X(24) X(25) X(27) X(30) X(36) X(40) X(45) X(48) X(50)                        \
    X(54) X(60) X(72) X(75) X(80) X(81) X(90) X(96) X(100) X(108) X(120) X(125) X(135) X(144) X(150) X(160)              \
    X(162) X(180) X(192) X(200) X(216) X(225) X(240) X(243) X(250) X(270) X(288) X(300) X(320) X(324) X(360) X(375)      \
    X(384) X(400) X(405) X(432) X(450) X(480) X(486) X(500) X(540) X(576) X(600) X(625) X(640) X(648) X(675) X(720)      \
    X(729) X(750) X(768) X(800) X(810) X(864) X(900) X(960) X(972) X(1000) X(1080) X(1125) X(1152) X(1200) X(1215) X(1250) \
    X(1280) X(1296) X(1350) X(1440) X(1458) X(1500) X(1536) X(1600) X(1620) X(1728) X(1800) X(1875) X(1920) X(1944) X(2000) X(2025)
#define REDIO_FFT_CT_SIZES_HI(X)                                                                                         \
    X(2160) X(2187) X(2250) X(2304) X(2400) X(2430) X(2500) X(2560) X(2592) X(2700) X(2880) X(2916) X(3000) X(3072) X(3125) X(3200) \
    X(3240) X(3375) X(3456) X(3600) X(3645) X(3750) X(3840) X(3888) X(4000) X(4050) X(4320) X(4374) X(4500) X(4608) X(4800) X(4860) \
    X(5000) X(5120) X(5184) X(5400) X(5625) X(5760) X(5832) X(6000) X(6075) X(6144) X(6250) X(6400) X(6480) X(6561) X(6750) X(6912) \
    X(7200) X(7290) X(7500) X(7680) X(7776) X(8000) X(8100)                                                              \
    X(8640) X(8748) X(9000) X(9216) X(9375) X(9600) X(9720) X(10000) X(10125) X(10240) X(10368) X(10800) X(10935) X(11250) X(11520) X(11664) \
    X(12000) X(12150) X(12288) X(12500) X(12800) X(12960) X(13122) X(13500) X(13824) X(14400) X(14580) X(15000) X(15360) X(15552) X(15625) X(16000) \
    X(16200)
#define REDIO_FFT_CT_SIZES(X) REDIO_FFT_CT_SIZES_LO(X) REDIO_FFT_CT_SIZES_HI(X)

inline bool fft_ct_size(int nfft)
{
    switch (nfft) {
#define REDIO_CT_CASE(NN) case NN:
        REDIO_FFT_CT_SIZES(REDIO_CT_CASE)
#undef REDIO_CT_CASE
        return true;
    default: return false;
    }
}

enum FftRoute {
    FFT_ROUTE_WAVE1K,      // fft1k_wave_kernel: 1024 points, one wavefront per transform
    FFT_ROUTE_P2,          // fft_p2_kernel: 2, 4, 8, 16, 32, 128, 512
    FFT_ROUTE_64,          // fft64_kernel
    FFT_ROUTE_256,         // fft256_kernel
    FFT_ROUTE_ONE_WAVE,    // fft2k_wave_kernel, fft4k_wave_kernel
    FFT_ROUTE_FOUR_WAVE,   // fft8k_wave_kernel, fft16k_wave_kernel
    FFT_ROUTE_CT,          // the compile-time list: fft_ct_kernel, fft_ct_wave_kernel, fft_ct_pair_kernel
    FFT_ROUTE_LDS_BATCHED, // fft_lds_batched_kernel: radices up to 5, at most 8192 points
    FFT_ROUTE_LDS,         // fft_lds_kernel: any size whose image (two images with a radix above 5) fits 128 KiB of LDS
    FFT_ROUTE_MULTIPASS,   // launch_fftbig: the powers of two from 2^15 to 2^24
    FFT_ROUTE_TILE_PASSES, // fft_tile_pass_kernel: radices up to 5 above 16384 points, powers of two excepted
    FFT_ROUTE_GLOBAL,      // fft_global_*: one launch per stage in global memory
};

struct FftRouteInfo {
    FftRoute route;
    bool in_place_ok; // false: the first pass is a global transposition, a call with in == out is staged through a copy of the input
    bool needs_work;  // true: a generic-radix stage in global memory runs out of place, a call needs nbatch * nfft elements of `work`
};

inline bool fft_multipass_size(int nfft) { return nfft >= (1 << 15) && nfft <= (1 << 24) && (nfft & (nfft - 1)) == 0 && nfft != 16384; }

// what follows the compile-time list in the cascade (the dispatcher also lands here for a listed size whose plan has no stage-ordered
// twiddle copy); generic: a radix above 5 among the stages
inline FftRouteInfo fft_route_unlisted(int nfft, bool generic)
{
    if (!generic && nfft <= 8192) return {FFT_ROUTE_LDS_BATCHED, true, false};
    if ((long)nfft * 8 * (generic ? 2 : 1) <= 128 * 1024) return {FFT_ROUTE_LDS, true, false}; // 8: sizeof(float2)
    if (fft_multipass_size(nfft)) return {FFT_ROUTE_MULTIPASS, false, false};
    // not a power of two: the tile passes read the stage-ordered twiddle copy, which a plan builds for exactly these sizes (2^25 and 2^26
    // have neither that copy nor the multi-pass tables)
    if (!generic && nfft > 16384 && (nfft & (nfft - 1)) != 0) return {FFT_ROUTE_TILE_PASSES, false, false};
    return {FFT_ROUTE_GLOBAL, false, generic};
}

template <typename Stage> // Stage: FftStage (fft_core.h); only the radix .p is read
inline FftRouteInfo fft_route(int nfft, const Stage *st, int nstages)
{
    switch (nfft) {
    case 1024: return {FFT_ROUTE_WAVE1K, true, false};
    case 2: case 4: case 8: case 16: case 32: case 128: case 512: return {FFT_ROUTE_P2, true, false};
    case 2048: return {FFT_ROUTE_ONE_WAVE, true, false};
    case 8192: return {FFT_ROUTE_FOUR_WAVE, true, false};
    case 64: return {FFT_ROUTE_64, true, false};
    case 256: return {FFT_ROUTE_256, true, false};
    case 4096: return {FFT_ROUTE_ONE_WAVE, true, false};
    case 16384: return {FFT_ROUTE_FOUR_WAVE, true, false};
    default: break;
    }
    if (fft_ct_size(nfft)) return {FFT_ROUTE_CT, true, false};
    bool generic = false;
    for (int i = 0; i < nstages; ++i) generic |= st[i].p > 5;
    return fft_route_unlisted(nfft, generic);
}

#pragma GCC visibility pop
} // namespace redio
