// ddc_kernels.hip -- gfx950 kernels of the tuner (include/redio.h, redio_ddc_*): kpn::mul_vecs by a periodic oscillator table
// (src/kpn/src/kpn.rs:198-203) fused into the tile load of dsputils::convolve (src/dsputils/src/dsputils.rs:30-32).
//
// Bound: HBM, as the FIR kernels (fir_kernels.hip): 8 + 8/D bytes per input sample from cf32, 2 + 8/D from the receiver's u8 I/Q
// bytes, against 32 + 8/D of redio_mul_c32 on a materialised oscillator followed by redio_fir_enqueue.  The kernels are the FIR's
// three tiled forms with another tile load (ddc_core.h): the loader multiplies every sample by its table entry on the way into the
// same padded LDS image, and fir_lane (fir_core.h) / fir_chunks (fir_chunks.h) run on that image unchanged.  The table is read
// through the vector cache with plain loads (every workgroup reads it: it stays in L2); the samples follow the FIR kernels'
// per-shape policy (non-temporal where they go by once: the chunked form at decimation >= 2).
#include "ddc_core.h"
#include "fir_chunks.h"
#include "redio_internal.h"

namespace redio {

// ---- specialised tiled kernel: the shapes of fir_tiled_kernel --------------------------------------------------------------------
template <bool U8, int K, int D, int R, bool FUSED, int NT>
__global__ __launch_bounds__(NT) void ddc_tiled_kernel(const void *__restrict__ x, long n_in, unsigned first_mod, const float2 *__restrict__ tab,
                                                       unsigned L, const float *__restrict__ taps, float2 *__restrict__ y, long n_out, int vec_in,
                                                       int vec_out)
{
    using G = FirGeom<K, D, R>;
    constexpr int TILE_OUT = NT * R, TILE_IN = G::tile_in(TILE_OUT);
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *xs = reinterpret_cast<float2 *>(smem);

    const long tile = blockIdx.x;
    const long in0 = tile * (long)TILE_OUT * D;
    const unsigned base = ddc_base(first_mod, (unsigned long long)in0, L); // wave-uniform: the workgroup's one modulo
    ddc_load_thread<U8, false>((int)threadIdx.x, NT, reinterpret_cast<const char *>(x) + in0 * (U8 ? 2 : 8), n_in - in0, tab + base, TILE_IN,
                               vec_in != 0, (base & 1u) == 0, [&](int n, float2 v) { xs[G::lds_index(n)] = v; });
    __syncthreads();

    float2 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = float2{};
    fir_lane<float2, K, D, R, FUSED>(xs, (int)threadIdx.x, taps, acc);

    const long o0 = tile * (long)TILE_OUT + (long)threadIdx.x * R;
    if (o0 + R <= n_out) {
        if (vec_out) { // y 16-byte aligned; o0 * 8 is a multiple of 16 (R even)
            float4 *y4 = reinterpret_cast<float4 *>(y + o0);
#pragma unroll
            for (int q = 0; q < R / 2; ++q) y4[q] = make_float4(acc[2 * q].x, acc[2 * q].y, acc[2 * q + 1].x, acc[2 * q + 1].y);
            return;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) y[o0 + r] = acc[r];
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (o0 + r < n_out) y[o0 + r] = acc[r];
    }
}

// ---- chunked tiled kernel: any tap count, the decimations of fir_chunked_kernel -----------------------------------------------------
template <bool U8, int D, int R, bool FUSED, int CHW>
__global__ __launch_bounds__(256) void ddc_chunked_kernel(const void *__restrict__ x, long n_in, unsigned first_mod, const float2 *__restrict__ tab,
                                                          unsigned L, const float *__restrict__ taps, int K, float2 *__restrict__ y, long n_out,
                                                          int vec_in, int vec_out)
{
    constexpr int NT = 256, TILE_OUT = NT * R, LSTR = R * D;
    constexpr bool PAD = (LSTR % 2) == 0;
    constexpr bool STREAM = D >= 2; // fir_chunked_kernel's policy: non-temporal tile loads and output stores where the samples go by once
    static_assert((R & (R - 1)) == 0 && R >= 2, "R is a power of two");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *xs = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    const int tile_in = (int)ddc_chunked_tile_in(K, D, R);
    const long t = blockIdx.x;
    const long in0 = t * TILE_OUT * D;
    const unsigned base = ddc_base(first_mod, (unsigned long long)in0, L); // wave-uniform: the workgroup's one modulo
    ddc_load_thread<U8, STREAM>(tid, NT, reinterpret_cast<const char *>(x) + in0 * (U8 ? 2 : 8), n_in - in0, tab + base, tile_in, vec_in != 0,
                                (base & 1u) == 0, [&](int n, float2 v) { xs[PAD ? n + n / LSTR : n] = v; });
    __syncthreads();
    float2 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = float2{};
    fir_chunks<float2, D, R, FUSED, CHW>(xs, tid * (LSTR + (PAD ? 1 : 0)), K, taps, acc);
    // outputs through LDS, as fir_chunked_kernel: element e of the tile sits at ys[(e / R) * (R + 1) + e % R]
    const long o0 = t * TILE_OUT;
    __syncthreads(); // every wave is done with the input tile
    float2 *ys = xs;
#pragma unroll
    for (int r = 0; r < R; ++r) ys[tid * (R + 1) + r] = acc[r];
    __syncthreads();
    const long left = n_out - o0; // outputs of this tile that exist
#pragma unroll
    for (int v = tid; v < TILE_OUT / 2; v += NT) {
        const int e0 = 2 * v;
        const float2 a = ys[(e0 / R) * (R + 1) + (e0 & (R - 1))], b = ys[((e0 + 1) / R) * (R + 1) + ((e0 + 1) & (R - 1))];
        if (vec_out && e0 + 2 <= left) {
            if constexpr (STREAM) __builtin_nontemporal_store(fir_v4f{a.x, a.y, b.x, b.y}, reinterpret_cast<fir_v4f *>(y + o0) + v);
            else reinterpret_cast<float4 *>(y + o0)[v] = make_float4(a.x, a.y, b.x, b.y);
        } else {
            if (e0 < left) y[o0 + e0] = a;
            if (e0 + 1 < left) y[o0 + e0 + 1] = b;
        }
    }
}

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
struct DdcArgs {
    const void *x; long n_in; unsigned first_mod; const float2 *tab; unsigned L; const float *taps; int K; long D; float2 *y; long n_out;
    int vec_in, vec_out; hipStream_t s;
};

template <bool U8, int K, int D, int R, bool FUSED>
hipError_t launch_tiled(const DdcArgs &a)
{
    constexpr int NT = 256, TILE_OUT = NT * R;
    using G = FirGeom<K, D, R>;
    constexpr size_t LDS = (size_t)G::lds_elems(TILE_OUT) * sizeof(float2);
    static_assert(LDS <= 160 * 1024, "tile does not fit LDS");
    static_assert(G::tile_in(TILE_OUT) + 2 <= DDC_TABLE_EXT, "a lane's table index stays inside the extended table");
    auto kern = ddc_tiled_kernel<U8, K, D, R, FUSED, NT>;
    if (LDS > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.n_out + TILE_OUT - 1) / TILE_OUT)), dim3(NT), LDS, a.s, a.x, a.n_in, a.first_mod, a.tab, a.L, a.taps, a.y,
                       a.n_out, a.vec_in, a.vec_out);
    return hipGetLastError();
}

template <bool U8, int D, bool FUSED>
hipError_t launch_chunked(const DdcArgs &a)
{
    constexpr int R = ddc_chunked_r(D), CHW = ddc_chunked_chw(D), TILE_OUT = 256 * R;
    const size_t lds = (size_t)ddc_chunked_lds_elems(a.K, D, R) * sizeof(float2);
    if ((long)lds > DDC_CHUNKED_LDS_MAX || ddc_chunked_tile_in(a.K, D, R) + 2 > DDC_TABLE_EXT) return hipErrorNotSupported; // ddc_route() sent it elsewhere
    auto kern = ddc_chunked_kernel<U8, D, R, FUSED, CHW>;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)((a.n_out + TILE_OUT - 1) / TILE_OUT)), dim3(256), lds, a.s, a.x, a.n_in, a.first_mod, a.tab, a.L, a.taps, a.K,
                       a.y, a.n_out, a.vec_in, a.vec_out);
    return hipGetLastError();
}

// routing mirrors launch_fir_t (fir_kernels.hip); ddc_route (ddc_core.h) is the same decision as a number
template <bool U8, bool FUSED>
hipError_t launch_ddc_t(const DdcArgs &a)
{
    const int K = a.K;
    const long D = a.D;
    switch (ddc_route(K, D)) {
    case 1:
        if (K == 127 && D == 5) return launch_tiled<U8, 127, 5, 4, FUSED>(a);
        if (K == 127 && D == 1) return launch_tiled<U8, 127, 1, 8, FUSED>(a);
        if (K == 63 && D == 1) return launch_tiled<U8, 63, 1, 8, FUSED>(a);
        return launch_tiled<U8, 63, 5, 4, FUSED>(a);
    case 2:
        switch (D) {
        case 1: return launch_chunked<U8, 1, FUSED>(a);
        case 2: return launch_chunked<U8, 2, FUSED>(a);
        case 3: return launch_chunked<U8, 3, FUSED>(a);
        case 4: return launch_chunked<U8, 4, FUSED>(a);
        case 5: return launch_chunked<U8, 5, FUSED>(a);
        case 8: return launch_chunked<U8, 8, FUSED>(a);
        case 10: return launch_chunked<U8, 10, FUSED>(a);
        default: return hipErrorNotSupported;
        }
    default: break;
    }
    hipLaunchKernelGGL((ddc_direct_kernel<U8, FUSED>), dim3((unsigned)((a.n_out + 255) / 256)), dim3(256), 0, a.s, a.x, a.first_mod, a.tab, a.L, a.taps, K, D,
                       a.y, a.n_out);
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
    const DdcArgs a = {x, n_in, first_mod, tab, L, taps, K, D, y, n_out, (reinterpret_cast<uintptr_t>(x) & (u8 ? 3 : 15)) == 0,
                       (reinterpret_cast<uintptr_t>(y) & 15) == 0, s};
    if (u8) return fused ? launch_ddc_t<true, true>(a) : launch_ddc_t<true, false>(a);
    return fused ? launch_ddc_t<false, true>(a) : launch_ddc_t<false, false>(a);
}

} // namespace redio
