// upfirdn_kernels.hip -- gfx950 kernels of the rational resampler (include/redio.h, redio_upfirdn_*): up by U, FIR, down by D as the
// polyphase form of dsputils::convolve (src/dsputils/src/dsputils.rs:30-32) over the original samples; contract in upfirdn_core.h.
//
// Bound: HBM, 8 + 8 D / U bytes per cf32 output (half that for f32), against the zero-stuffed composition's U-times stream written,
// read again and multiplied by zeros.  Route 1 stages a tile once and walks the U' phases over it (lanes are periods, so a phase's
// taps are wave-uniform and come by scalar loads); route 2 is one output per thread for every other shape.
#include "upfirdn_core.h"
#include "redio_internal.h"

namespace redio {

// ---- route 1: the phase-walking tiled kernel.  D = D' from the chunked FIR's set, R periods per lane, U' at run time ----------------
template <typename T, int D, int R, bool FUSED, int CHW>
__global__ __launch_bounds__(256) void upfirdn_tiled_kernel(const T *__restrict__ x, long n_in, const UpfirdnPhase *__restrict__ ph,
                                                            const float *__restrict__ taps, int Up, int Wp, T *__restrict__ y, long n_out, int vec_in,
                                                            int vec_out)
{
    constexpr int NT = 256, NQ = NT * R, LSTR = R * D;
    constexpr bool STREAM = D >= 2; // fir_chunked_kernel's policy: non-temporal tile loads and output stores where the samples go by once
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    T *ys = xs + upfirdn_img_elems(R, D, Wp); // the output tile: NQ * Up elements, 16-byte aligned
    const int tid = threadIdx.x;
    const long t = blockIdx.x;
    const long in0 = t * NQ * D;
    upfirdn_load_thread<T, STREAM>(tid, NT, x + in0, n_in - in0, (int)upfirdn_tile_in(R, D, Wp), vec_in != 0,
                                   [&](int n, T v) { xs[tile_image_index(n, LSTR)] = v; });
    __syncthreads();
    upfirdn_phases_thread<T, D, R, FUSED, CHW>(xs, ys, tid, ph, taps, Up);
    __syncthreads();
    const long o0 = t * NQ * Up; // o0 * sizeof(T) is a multiple of 16
    upfirdn_store_thread<T, STREAM>(tid, NT, ys, NQ * Up, y + o0, n_out - o0, vec_out != 0);
}

// ---- route 2: the direct kernel, any U, D and K; one output per thread -----------------------------------------------------------------
template <typename T, bool FUSED>
__global__ __launch_bounds__(256) void upfirdn_direct_kernel(const T *__restrict__ x, const UpfirdnPhase *__restrict__ ph, const float *__restrict__ taps,
                                                             long Up, long Dp, T *__restrict__ y, long n_out)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_out) return;
    y[i] = upfirdn_direct_output<T, FUSED>(x, i, Up, Dp, ph, taps);
}

namespace {
struct UpfirdnArgs {
    const void *x; long n_in; const UpfirdnPhase *ph; const float *taps; long K, U, D; void *y; long n_out; hipStream_t s;
};

template <typename T, int D, int R, bool FUSED>
hipError_t launch_tiled(const UpfirdnArgs &a)
{
    constexpr int NQ = 256 * R;
    const long Up = upfirdn_period_out(a.U, a.D), Wp = upfirdn_window(a.K, a.U, a.D);
    const size_t lds = (size_t)upfirdn_lds_elems(R, Up, D, Wp) * sizeof(T);
    if ((long)lds > UPFIRDN_LDS_MAX) return hipErrorNotSupported; // upfirdn_route() sent it elsewhere
    auto kern = upfirdn_tiled_kernel<T, D, R, FUSED, 16>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int vec_in = (reinterpret_cast<uintptr_t>(a.x) & 15) == 0, vec_out = (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;
    const long per_tile = NQ * Up;
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.n_out + per_tile - 1) / per_tile)), dim3(256), lds, a.s, static_cast<const T *>(a.x), a.n_in, a.ph,
                       a.taps, (int)Up, (int)Wp, static_cast<T *>(a.y), a.n_out, vec_in, vec_out);
    return hipGetLastError();
}

template <typename T, int D, bool FUSED>
hipError_t launch_tiled_r(const UpfirdnArgs &a)
{
    switch (upfirdn_r(a.K, a.U, a.D)) {
    case 4:
        if constexpr (upfirdn_r_max(D) >= 4) return launch_tiled<T, D, 4, FUSED>(a);
        return hipErrorNotSupported;
    case 2: return launch_tiled<T, D, 2, FUSED>(a);
    case 1: return launch_tiled<T, D, 1, FUSED>(a);
    default: return hipErrorNotSupported;
    }
}

template <typename T, bool FUSED>
hipError_t launch_upfirdn_t(const UpfirdnArgs &a)
{
    const long Up = upfirdn_period_out(a.U, a.D), Dp = upfirdn_period_in(a.U, a.D);
    if (upfirdn_route(a.K, a.U, a.D) == 1)
        return tile_dispatch_d(Dp, hipErrorNotSupported, [&](auto d) { return launch_tiled_r<T, decltype(d)::value, FUSED>(a); });
    hipLaunchKernelGGL((upfirdn_direct_kernel<T, FUSED>), dim3((unsigned)((a.n_out + 255) / 256)), dim3(256), 0, a.s, static_cast<const T *>(a.x), a.ph,
                       a.taps, Up, Dp, static_cast<T *>(a.y), a.n_out);
    return hipGetLastError();
}
} // namespace

// x: n_in samples (f32, or cf32 with cplx); ph / taps: the plan's phase table and polyphase taps (upfirdn_core.h); y: n_out > 0 outputs,
// every one of them with its whole window inside the n_in samples (the caller's check).  Any whole-sample alignment: 16-byte aligned x
// takes the wide loads, 16-byte aligned y the wide stores.
hipError_t launch_upfirdn(const void *x, long n_in, const UpfirdnPhase *ph, const float *taps, long K, long U, long D, void *y, long n_out, bool cplx,
                          bool fused, hipStream_t s)
{
    if (n_out <= 0) return hipSuccess;
    const UpfirdnArgs a = {x, n_in, ph, taps, K, U, D, y, n_out, s};
    if (cplx) return fused ? launch_upfirdn_t<float2, true>(a) : launch_upfirdn_t<float2, false>(a);
    return fused ? launch_upfirdn_t<float, true>(a) : launch_upfirdn_t<float, false>(a);
}

} // namespace redio
