// fir_tile_kernels.h -- the two tiled kernel bodies of the FIR and their launchers, with the tile loader as a policy: fir_kernels.hip
// instantiates them with the plain loader (PlainTile below), ddc_kernels.hip with the tuner's (DdcTile, ddc_core.h), which multiplies
// every sample by its oscillator entry on the way into the same image.  Geometry, loader and store epilogues: fir_tile.h.
//
// A loader policy is a trivially copyable kernel argument with
//   sample_t                                        the sample type T of the image and the outputs
//   load<STREAM, LB>(tid, in0, tile_in, put)        thread tid's share of the tile whose first sample is in0: tile sample n through put(n, v)
#pragma once
#include "fir_chunks.h"
#include "fir_core.h"
#include "fir_tile.h"
#include "redio_internal.h"

namespace redio {

template <typename T>
struct PlainTile {
    using sample_t = T;
    const T *x; long n_in; int vec_in; // vec_in: x is 16-byte aligned
    template <bool STREAM, int LB, typename Put>
    RD_D void load(int tid, long in0, int tile_in, Put &&put) const
    {
        tile_load_thread<T, STREAM, LB>(tid, 256, x + in0, n_in - in0, tile_in, vec_in != 0, put);
    }
};

// ---- specialised tiled kernel: compile-time taps, the lane program of fir_core.h, lane-owned outputs --------------------------------
template <typename Load, int K, int D, int R, bool FUSED, int NT>
__global__ __launch_bounds__(NT) void fir_tiled_kernel(const Load in, const float *__restrict__ taps, typename Load::sample_t *__restrict__ y,
                                                       long n_out, int vec_out)
{
    using T = typename Load::sample_t;
    using G = FirGeom<K, D, R>;
    constexpr int TILE_OUT = NT * R, TILE_IN = G::tile_in(TILE_OUT);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *xs = reinterpret_cast<T *>(smem);

    const long tile = blockIdx.x;
    const int tid = threadIdx.x;
    in.template load<false, 0>(tid, tile * (long)TILE_OUT * D, TILE_IN, [&](int n, auto v) {
        if constexpr (std::is_same_v<decltype(v), float4>) { // the samples of one 16-byte load
#pragma unroll
            for (int e = 0; e < 16 / (int)sizeof(T); ++e) xs[G::lds_index(n + e)] = tile_elem<T>(v, e);
        } else {
            xs[G::lds_index(n)] = v;
        }
    });
    __syncthreads();

    T acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = T{};
    fir_lane<T, K, D, R, FUSED>(xs, tid, taps, acc);
    tile_store_lane<T, R>(acc, y, tile * (long)TILE_OUT + (long)tid * R, n_out, vec_out != 0);
}

template <typename Load, int K, int D, int R, bool FUSED>
static hipError_t launch_tiled(const Load &in, const float *taps, typename Load::sample_t *y, long n_out, hipStream_t s)
{
    using T = typename Load::sample_t;
    constexpr int NT = 256;
    using G = FirGeom<K, D, R>;
    constexpr int TILE_OUT = NT * R;
    constexpr size_t LDS = (size_t)G::lds_elems(TILE_OUT) * sizeof(T);
    static_assert(LDS <= 160 * 1024, "tile does not fit LDS");
    auto kern = fir_tiled_kernel<Load, K, D, R, FUSED, NT>;
    if (LDS > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
        if (e != hipSuccess) return e;
    }
    const int vec_out = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_out + TILE_OUT - 1) / TILE_OUT)), dim3(NT), LDS, s, in, taps, y, n_out, vec_out);
    return hipGetLastError();
}

// ---- chunked tiled kernel: any tap count, the decimations of the table (fir_tile.h), fir_chunks, outputs through LDS -----------------
// Memory side (round 2; the skeleton alone -- tile in, tile out, no arithmetic -- ran at 2.9 TB/s with 8-byte loads and each lane
// storing its R consecutive outputs; 5.5 TB/s now): the tile arrives as 16-byte loads, and the outputs leave through an LDS
// transpose (lane writes its R results at a stride of R + 1 elements, conflict-free; the workgroup reads them back in output
// order) so that every store instruction writes 1 KiB of consecutive bytes.  A persistent form (a workgroup walks tiles with the
// next tile's loads in flight during the arithmetic) was built and measured slower -- at 64 taps / 1 the tile's LDS traffic
// (237 KB: window reads, tile, transpose) and its multiply-adds each fill most of the time on their own, and fewer resident waves
// hide less of it: profiles/r02_fir_generic_experiments.txt.
// Round 3, again for the shapes HBM binds (decimation >= 3): a resident grid, each workgroup walking tiles with the first rounds of the
// NEXT tile's 16-byte loads issued right after the current tile's image is complete (in flight during its arithmetic and stores):
// slower on 7 of 8 shapes (101 taps / 3: 0.197 ms against 0.154; 255 / 10: 0.185 against 0.178).  profiles/r03_fir_chunked.txt.
template <typename Load, int D, bool FUSED>
__global__ __launch_bounds__(256) void fir_chunked_kernel(const Load in, const float *__restrict__ taps, int K,
                                                          typename Load::sample_t *__restrict__ y, long n_out, int vec_out)
{
    using T = typename Load::sample_t;
    constexpr int NT = 256, R = tile_r(D), CHW = tile_chw(D), TILE_OUT = NT * R, LSTR = R * D, VEC = 16 / (int)sizeof(T);
    // non-temporal tile loads and output stores where the samples go by once (round 3, per shape, both together: 31 taps / 2 -8 %, 255 / 10
    // -5 %, 129 / 8 -4 %, 101 / 3 and 200 / 4 unchanged); without decimation the loads alone cost 8 % at 64 taps, so D = 1 keeps the default policy
    constexpr bool STREAM = D >= 2;
    // the plain loader's whole-tile path: eight loads in flight per lane.  Round 3: its guarded loop keeps four in flight and waits three
    // times for a 43 KB tile (255 taps / 10); here every wait covers eight
    constexpr int LB = 8;
    static_assert(tile_table_ok(D), "the samples of one 16-byte load share one pad count; R is a power of two");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    T *xs = reinterpret_cast<T *>(smem);
    const int tid = threadIdx.x;
    const long t = blockIdx.x; // the tile
    in.template load<STREAM, LB>(tid, t * TILE_OUT * D, (int)tile_in(R, D, tile_window(K)), [&](int n, auto v) {
        T *d = xs + tile_image_index(n, LSTR);
        if constexpr (std::is_same_v<decltype(v), float4>) { // the VEC samples of one load, side by side (tile_table_ok)
#pragma unroll
            for (int e = 0; e < VEC; ++e) d[e] = tile_elem<T>(v, e);
        } else {
            *d = v;
        }
    });
    __syncthreads();
    T acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = T{};
    fir_chunks<T, D, R, FUSED, CHW>(xs, tile_lane_base(tid, LSTR), K, taps, acc);
    __syncthreads(); // every wave is done with the input tile: the transpose reuses it
    tile_transpose_put<T, R>(xs, tid, acc);
    __syncthreads();
    const long o0 = t * TILE_OUT;
    tile_store_thread<T, STREAM>(tid, NT, xs, TILE_OUT, y + o0, n_out - o0, vec_out != 0, [](int e) { return tile_transpose_index(e, R); });
}

// hipErrorNotSupported where the tile cannot fit LDS
template <typename Load, int D, bool FUSED>
static hipError_t launch_chunked(const Load &in, const float *taps, int K, typename Load::sample_t *y, long n_out, hipStream_t s)
{
    using T = typename Load::sample_t;
    constexpr int R = tile_r(D), TILE_OUT = 256 * R;
    const size_t lds = (size_t)tile_lds_elems(R, D, tile_window(K)) * sizeof(T);
    if (lds > (size_t)TILE_LDS_MAX) return hipErrorNotSupported;
    auto kern = fir_chunked_kernel<Load, D, FUSED>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const int vec_out = (reinterpret_cast<uintptr_t>(y) & 15) == 0;
    hipLaunchKernelGGL(kern, dim3((unsigned)((n_out + TILE_OUT - 1) / TILE_OUT)), dim3(256), lds, s, in, taps, K, y, n_out, vec_out);
    return hipGetLastError();
}

} // namespace redio
