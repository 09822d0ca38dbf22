// ddc_upfirdn_kernels.hip -- gfx950 kernels of the tuned resampler (include/redio.h, redio_ddc_upfirdn_*): kpn::mul_vecs by a periodic
// oscillator table (src/kpn/src/kpn.rs:198-203) fused into the tile load of the rational resampler, the polyphase form of
// dsputils::convolve (src/dsputils/src/dsputils.rs:30-32); contract in ddc_upfirdn_core.h.
//
// Bound: HBM, 8 + 8 D / U bytes per output from cf32 and 8 + 2 D / U from the receiver's u8 I/Q bytes, against 24 more bytes per input
// sample of redio_mul_c32 on a materialised oscillator followed by redio_upfirdn_enqueue.  Route 1 is the resampler's tiled kernel body
// (upfirdn_tile_kernels.h) with the tuner's loader (ddc_core.h, DdcTile) as its policy: the mixed samples go into the same padded LDS
// image, and the phase loop and the store loop run on it unchanged.  The table is read through the vector cache with plain loads (every
// workgroup reads it: it stays in L2).  Route 2 is one output per thread.
#include "ddc_upfirdn_core.h"
#include "upfirdn_tile_kernels.h"

namespace redio {

// ---- route 2: the direct kernel, any U, D and K; one output per thread -----------------------------------------------------------------
template <bool U8, bool FUSED>
__global__ __launch_bounds__(256) void ddc_upfirdn_direct_kernel(const void *__restrict__ x, unsigned first_mod, const float2 *__restrict__ tab, unsigned L,
                                                                 const UpfirdnPhase *__restrict__ ph, const float *__restrict__ taps, long Up, long Dp,
                                                                 float2 *__restrict__ y, long n_out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    y[i] = ddc_upfirdn_direct_output<U8, FUSED>(x, i, Up, Dp, ph, taps, first_mod, tab, L);
}

namespace {
template <bool U8, bool FUSED>
hipError_t launch_ddc_upfirdn_t(const DdcTile<U8> &in, const UpfirdnTileArgs &a)
{
    const long Up = upfirdn_period_out(a.U, a.D), Dp = upfirdn_period_in(a.U, a.D);
    if (upfirdn_route(a.K, a.U, a.D) == 1) {
        // a lane's table index would leave the extended table: no shape route 1 takes (ddc_upfirdn_core.h's static_assert), checked all the same
        if (!ddc_upfirdn_tile_ok(upfirdn_r(a.K, a.U, a.D), Dp, upfirdn_window(a.K, a.U, a.D))) return hipErrorNotSupported;
        return launch_upfirdn_route1<DdcTile<U8>, FUSED>(in, a);
    }
    hipLaunchKernelGGL((ddc_upfirdn_direct_kernel<U8, FUSED>), dim3((unsigned)((a.n_out + 255) / 256)), dim3(256), 0, a.s, in.x, in.first_mod, in.tab, in.L,
                       a.ph, a.taps, Up, Dp, static_cast<float2 *>(a.y), a.n_out);
    return hipGetLastError();
}
} // namespace

// x: n_in cf32 samples, or with u8 their 2 * n_in interleaved I/Q bytes; tab: the plan's device table (period L, extended by
// DDC_TABLE_EXT entries); first_mod = first_index mod L; ph / taps: the phase table and polyphase taps (upfirdn_core.h) for K taps, up U,
// down D; y: n_out > 0 outputs, every one of them with its whole window inside the n_in samples (the caller's check).  Any pointer
// alignment (a whole cf32 sample; any byte): the two-samples-per-load path needs x 16-byte (u8: 4-byte) aligned, the 16-byte stores y
// 16-byte aligned.
hipError_t launch_ddc_upfirdn(const void *x, bool u8, long n_in, unsigned first_mod, const float2 *tab, unsigned L, const UpfirdnPhase *ph, const float *taps,
                              long K, long U, long D, float2 *y, long n_out, bool fused, hipStream_t s)
{
    if (n_out <= 0) return hipSuccess;
    const int vec_in = (reinterpret_cast<uintptr_t>(x) & (u8 ? 3 : 15)) == 0;
    const UpfirdnTileArgs a = {ph, taps, K, U, D, y, n_out, s};
    if (u8) {
        const DdcTile<true> in = {x, n_in, first_mod, tab, L, vec_in};
        return fused ? launch_ddc_upfirdn_t<true, true>(in, a) : launch_ddc_upfirdn_t<true, false>(in, a);
    }
    const DdcTile<false> in = {x, n_in, first_mod, tab, L, vec_in};
    return fused ? launch_ddc_upfirdn_t<false, true>(in, a) : launch_ddc_upfirdn_t<false, false>(in, a);
}

} // namespace redio
