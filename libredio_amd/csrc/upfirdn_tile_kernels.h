// upfirdn_tile_kernels.h -- route 1 of the rational resampler with the tile loader as a policy (fir_tile_kernels.h describes one):
// the phase-walking tiled kernel body and its launchers.  ddc_upfirdn_kernels.hip instantiates them with the tuner's loader
// (DdcTile<U8>, ddc_core.h), which multiplies every sample by its oscillator entry on the way into the same image; the phase loop and
// the store loop (upfirdn_core.h) run on that image unchanged.
//
// The resampler's own kernel (upfirdn_kernels.hip, upfirdn_tiled_kernel) is this body with the plain loader written in place.  It
// stays as it is: instantiated from here with PlainTile<T> every one of its 76 instances kept its VGPRs, scratch and LDS but took one
// or two SGPRs fewer (the loader's arguments arrive as one kernel-argument struct), and the plan's figures are pinned
// (profiles/r17_ddc_upfirdn_resources.txt).  A change to the body belongs in both.
#pragma once
#include "fir_tile.h"
#include "redio_internal.h"
#include "upfirdn_core.h"

namespace redio {

// D = D' from the chunked FIR's set, R periods per lane, U' at run time.  The sink takes single samples, or the samples of one 16-byte
// load one by one: a lane stride of 2 or 4 samples (R = 1) does not keep them side by side.  LB = 4 is what a plain loader would keep
// in flight; DdcTile keeps its own count
template <typename Load, int D, int R, bool FUSED, int CHW>
__global__ __launch_bounds__(256) void upfirdn_policy_tiled_kernel(const Load in, const UpfirdnPhase *__restrict__ ph, const float *__restrict__ taps, int Up,
                                                                   int Wp, typename Load::sample_t *__restrict__ y, long n_out, int vec_out)
{
    using T = typename Load::sample_t;
    constexpr int NT = 256, NQ = NT * R, LSTR = R * D;
    constexpr bool STREAM = D >= 2; // fir_chunked_kernel's policy: non-temporal tile loads and output stores where the samples go by once
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    T *ys = xs + upfirdn_img_elems(R, D, Wp); // the output tile: NQ * Up elements, 16-byte aligned
    const int tid = threadIdx.x;
    const long t = blockIdx.x;
    const long in0 = t * NQ * D; // a multiple of 256 samples: the alignment of the call's first sample is every tile's
    in.template load<STREAM, 4>(tid, in0, (int)upfirdn_tile_in(R, D, Wp), [&](int n, auto v) {
        if constexpr (std::is_same_v<decltype(v), float4>) {
#pragma unroll
            for (int e = 0; e < 16 / (int)sizeof(T); ++e) xs[tile_image_index(n + e, LSTR)] = tile_elem<T>(v, e);
        } else {
            xs[tile_image_index(n, LSTR)] = v;
        }
    });
    __syncthreads();
    upfirdn_phases_thread<T, D, R, FUSED, CHW>(xs, ys, tid, ph, taps, Up);
    __syncthreads();
    const long o0 = t * NQ * Up; // o0 * sizeof(T) is a multiple of 16
    upfirdn_store_thread<T, STREAM>(tid, NT, ys, NQ * Up, y + o0, n_out - o0, vec_out != 0);
}

// what the launchers take beside the loader: the plan's tables and shape, the outputs
struct UpfirdnTileArgs {
    const UpfirdnPhase *ph; const float *taps; long K, U, D; void *y; long n_out; hipStream_t s;
};

template <typename Load, int D, int R, bool FUSED>
static hipError_t launch_upfirdn_tiled(const Load &in, const UpfirdnTileArgs &a)
{
    using T = typename Load::sample_t;
    constexpr int NQ = 256 * R;
    const long Up = upfirdn_period_out(a.U, a.D), Wp = upfirdn_window(a.K, a.U, a.D);
    const size_t lds = (size_t)upfirdn_lds_elems(R, Up, D, Wp) * sizeof(T);
    if ((long)lds > UPFIRDN_LDS_MAX) return hipErrorNotSupported; // upfirdn_route() sent it elsewhere
    auto kern = upfirdn_policy_tiled_kernel<Load, D, R, FUSED, 16>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int vec_out = (reinterpret_cast<uintptr_t>(a.y) & 15) == 0;
    const long per_tile = NQ * Up;
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.n_out + per_tile - 1) / per_tile)), dim3(256), lds, a.s, in, a.ph, a.taps, (int)Up, (int)Wp,
                       static_cast<T *>(a.y), a.n_out, vec_out);
    return hipGetLastError();
}

template <typename Load, int D, bool FUSED>
static hipError_t launch_upfirdn_tiled_r(const Load &in, const UpfirdnTileArgs &a)
{
    switch (upfirdn_r(a.K, a.U, a.D)) {
    case 4:
        if constexpr (upfirdn_r_max(D) >= 4) return launch_upfirdn_tiled<Load, D, 4, FUSED>(in, a);
        return hipErrorNotSupported;
    case 2: return launch_upfirdn_tiled<Load, D, 2, FUSED>(in, a);
    case 1: return launch_upfirdn_tiled<Load, D, 1, FUSED>(in, a);
    default: return hipErrorNotSupported;
    }
}

// a call whose route is 1: D' as a compile-time constant, then R
template <typename Load, bool FUSED>
static hipError_t launch_upfirdn_route1(const Load &in, const UpfirdnTileArgs &a)
{
    return tile_dispatch_d(upfirdn_period_in(a.U, a.D), hipErrorNotSupported,
                           [&](auto d) { return launch_upfirdn_tiled_r<Load, decltype(d)::value, FUSED>(in, a); });
}

} // namespace redio
