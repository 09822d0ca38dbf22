// ddc_kernels.hip -- gfx950 kernels of the tuner (include/redio.h, redio_ddc_*): kpn::mul_vecs by a periodic oscillator table
// (src/kpn/src/kpn.rs:198-203) fused into the tile load of dsputils::convolve (src/dsputils/src/dsputils.rs:30-32).
//
// Bound: HBM, as the FIR kernels (fir_kernels.hip): 8 + 8/D bytes per input sample from cf32, 2 + 8/D from the receiver's u8 I/Q
// bytes, against 32 + 8/D of redio_mul_c32 on a materialised oscillator followed by redio_fir_enqueue.  The tiled kernels are the FIR's
// own bodies (fir_tile_kernels.h: fir_tiled_kernel, fir_chunked_kernel) instantiated with the tuner's loader (ddc_core.h, DdcTile): it
// multiplies every sample by its table entry on the way into the same padded LDS image, and fir_lane (fir_core.h) / fir_chunks
// (fir_chunks.h) run on that image unchanged.  The table is read through the vector cache with plain loads (every workgroup reads it: it
// stays in L2); the samples follow the FIR kernels' per-shape policy (non-temporal where they go by once: the chunked form at
// decimation >= 2).  Only the direct kernel is the tuner's own.
#include "ddc_core.h"
#include "fir_tile_kernels.h"

namespace redio {

// ---- direct kernel: any K and D, no tile; one output per thread ---------------------------------------------------------------------
template <bool U8, bool FUSED>
__global__ __launch_bounds__(256) void ddc_direct_kernel(const void *__restrict__ x, unsigned first_mod, const float2 *__restrict__ tab, unsigned L,
                                                         const float *__restrict__ taps, int K, long D, float2 *__restrict__ y, long n_out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    const unsigned idx0 = ddc_base(first_mod, (unsigned long long)(i * D), L); // one modulo per thread, then wrap by compare
    y[i] = ddc_direct_output<U8, FUSED>(reinterpret_cast<const char *>(x) + i * D * (U8 ? 2 : 8), idx0, tab, L, taps, K);
}

namespace {
// routing mirrors launch_fir_t (fir_kernels.hip); ddc_route (ddc_core.h) is the same decision as a number
template <bool U8, bool FUSED>
hipError_t launch_ddc_t(const DdcTile<U8> &in, const float *taps, int K, long D, float2 *y, long n_out, hipStream_t s)
{
    using L = DdcTile<U8>;
    switch (ddc_route(K, D)) {
    case 1:
        static_assert(FirGeom<127, 1, 8>::tile_in(256 * 8) + 2 <= DDC_TABLE_EXT && FirGeom<127, 5, 4>::tile_in(256 * 4) + 2 <= DDC_TABLE_EXT,
                      "a lane's table index stays inside the extended table");
        if (K == 127 && D == 5) return launch_tiled<L, 127, 5, 4, FUSED>(in, taps, y, n_out, s);
        if (K == 127 && D == 1) return launch_tiled<L, 127, 1, 8, FUSED>(in, taps, y, n_out, s);
        if (K == 63 && D == 1) return launch_tiled<L, 63, 1, 8, FUSED>(in, taps, y, n_out, s);
        return launch_tiled<L, 63, 5, 4, FUSED>(in, taps, y, n_out, s);
    case 2:
        return tile_dispatch_d(D, hipErrorNotSupported, [&](auto d) {
            constexpr int DD = decltype(d)::value;
            if (ddc_chunked_tile_in(K, DD, ddc_chunked_r(DD)) + 2 > DDC_TABLE_EXT) return hipErrorNotSupported; // a lane's table index would leave the extended table
            return launch_chunked<L, DD, FUSED>(in, taps, K, y, n_out, s);
        });
    default: break;
    }
    hipLaunchKernelGGL((ddc_direct_kernel<U8, FUSED>), dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, s, in.x, in.first_mod, in.tab, in.L, taps, K, D, y,
                       n_out);
    return hipGetLastError();
}
} // namespace

// x: n_in cf32 samples, or with u8 their 2 * n_in interleaved I/Q bytes; tab: the plan's device table (period L, extended by
// DDC_TABLE_EXT entries); first_mod = first_index mod L; y: n_out > 0 outputs.  Any pointer alignment (a whole cf32 sample; any byte):
// the two-samples-per-load path needs x 16-byte (u8: 4-byte) aligned, the 16-byte stores y 16-byte aligned.
hipError_t launch_ddc(const void *x, bool u8, long n_in, unsigned first_mod, const float2 *tab, unsigned L, const float *taps, int K, long D, float2 *y,
                      long n_out, bool fused, hipStream_t s)
{
    if (n_out <= 0) return hipSuccess;
    const int vec_in = (reinterpret_cast<uintptr_t>(x) & (u8 ? 3 : 15)) == 0;
    if (u8) {
        const DdcTile<true> in = {x, n_in, first_mod, tab, L, vec_in};
        return fused ? launch_ddc_t<true, true>(in, taps, K, D, y, n_out, s) : launch_ddc_t<true, false>(in, taps, K, D, y, n_out, s);
    }
    const DdcTile<false> in = {x, n_in, first_mod, tab, L, vec_in};
    return fused ? launch_ddc_t<false, true>(in, taps, K, D, y, n_out, s) : launch_ddc_t<false, false>(in, taps, K, D, y, n_out, s);
}

} // namespace redio
