// ovsave_real_kernels.hip -- gfx950 kernels of overlap-save on REAL streams (redio_ovsave_real_*; contract: DESIGN.md 5.7b).
//
// Bound: HBM.  Two strategies:
//   ovsave_real2k_kernel   N = 2048: one wavefront per block keeps the block in registers from its load to the store of its hop
//                          outputs -- the one-wave transform of fft_wave.h, the forward split of fftr_core.h into registers, the
//                          product with conj(H), the inverse split and the inverse transform.  4 N / hop + 4 bytes per output.
//   the small kernels below  every other even N: the product and the scaled copy between the plan's two redio_fftr transforms
//                          (ovsave_real_api.hip), and the row gather for input that is only 4-byte aligned.
#include "redio_internal.h"
#include "fft_wave.h"
#include "ovsave_real_core.h"

namespace redio {

// One wavefront per block, OVSR2K_RUN consecutive blocks per wavefront, the next block's samples loaded under this block's
// arithmetic (the schedule of fftr1k_fwd_kernel).  ALIGNED: x + b hop is 8-byte aligned (every caller but a carried stream whose
// message started on an odd sample); otherwise the pair is two 4-byte loads of the same samples.
constexpr int OVSR2K_RUN = 4;

template <bool ALIGNED>
__device__ __forceinline__ void ovsr2k_load(float2 (&v)[16], const float *row, int lane)
{
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int p = lane + 64 * i;
        if (ALIGNED) v[i] = reinterpret_cast<const float2 *>(row)[p];
        else v[i] = make_float2(row[2 * p], row[2 * p + 1]);
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(256) void ovsave_real2k_kernel(const float *__restrict__ x, long hop, const float2 *__restrict__ tw_f,
                                                            const float2 *__restrict__ tw_i, const float2 *__restrict__ stw_f,
                                                            const float2 *__restrict__ stw_i, const float2 *__restrict__ Hc,
                                                            float *__restrict__ out, long nblk, float scale)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *ex = reinterpret_cast<float2 *>(smem) + wave * FFT1K_LDS;
    const long b0 = ((long)blockIdx.x * 4 + wave) * OVSR2K_RUN;
    if (b0 >= nblk) return; // wave-uniform
    const long b1 = (b0 + OVSR2K_RUN < nblk) ? b0 + OVSR2K_RUN : nblk;
    Fft1kTw tf, ti;
    fft1k_load_tw(tf, lane, tw_f);
    fft1k_load_tw(ti, lane, tw_i);
    Fftr1kTw wf, wi;
    fftr1k_load_tw(wf, lane, stw_f);
    fftr1k_load_tw(wi, lane, stw_i);
    float2 v[16], nx[16];
    ovsr2k_load<ALIGNED>(v, x + b0 * hop, lane);
    for (long b = b0; b < b1; ++b) {
        const long bn = (b + 1 < b1) ? b + 1 : b;
        ovsr2k_load<ALIGNED>(nx, x + bn * hop, lane);
        fft1k_wave_stages0to3<false>(v, ex, tw_f, tf, lane);
        fft1k_passC<false>(v, tf);
        wave_lds_fence(); // every lane has read its last-stage inputs before Z overwrites the image
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) ex[lane + 64 * q + 256 * j] = v[4 * q + j];
        wave_lds_fence();
        float2 a[8], c[8], mid;
        fftr1k_post_lane_regs(v, ex, wf, lane, a, c, mid);
        ovsr1k_product(a, c, mid, Hc, lane); // 8.2 KB table: L1-resident
        wave_lds_fence(); // every lane has read its partner Z before the inverse split overwrites slots 512 ... 1023
        fftr1k_pre_lane(a, c, mid, wi, lane, v, ex);
        wave_lds_fence();
        fftr1k_pre_gather(v, ex, lane);
        fft1k_wave_stages0to3<true>(v, ex, tw_i, ti, lane);
        fft1k_passC<true>(v, ti);
        ovsr1k_store(v, reinterpret_cast<float2 *>(out + b * hop), lane, hop, scale);
        wave_lds_fence();
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = nx[i];
    }
}

hipError_t launch_ovsave_real2k(const float *x, long hop, const float2 *tw_f, const float2 *tw_i, const float2 *stw_f, const float2 *stw_i,
                                const float2 *Hc, float *out, long nblk, float scale, hipStream_t s)
{
    if (nblk <= 0) return hipSuccess;
    const size_t lds = 4 * FFT1K_LDS * sizeof(float2);
    const long g = (nblk + 4 * OVSR2K_RUN - 1) / (4 * OVSR2K_RUN);
    if (g > 0x7fffffffl) return hipErrorInvalidValue;
    if (((uintptr_t)x & 7) == 0)
        hipLaunchKernelGGL(ovsave_real2k_kernel<true>, dim3((unsigned)g), dim3(256), lds, s, x, hop, tw_f, tw_i, stw_f, stw_i, Hc, out, nblk, scale);
    else
        hipLaunchKernelGGL(ovsave_real2k_kernel<false>, dim3((unsigned)g), dim3(256), lds, s, x, hop, tw_f, tw_i, stw_f, stw_i, Hc, out, nblk, scale);
    return hipGetLastError();
}

// ---- every other size ----------------------------------------------------------------------------
// rows of nbins = N / 2 + 1 bins, in place: S[row][k] *= Hc[k]
__global__ __launch_bounds__(256) void ovsave_real_mul_kernel(float2 *S, const float2 *__restrict__ Hc, long total, int nbins)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    S[i] = cmul_rn(S[i], Hc[i % nbins]);
}
__global__ __launch_bounds__(256) void ovsave_real_conj_kernel(float2 *H, int nbins)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nbins) H[i].y = -H[i].y;
}
// the first hop samples of each row of nfft, scaled; pairs (hop and nfft are even, both sides 8-byte aligned)
__global__ __launch_bounds__(256) void ovsave_real_scale_out_kernel(const float2 *__restrict__ y, float2 *__restrict__ out, long nblk, long half_nfft,
                                                                    long half_hop, float scale)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblk * half_hop) return;
    const long b = i / half_hop, r = i - b * half_hop;
    const float2 v = y[b * half_nfft + r];
    out[i] = make_float2(mul_rn(v.x, scale), mul_rn(v.y, scale));
}
// row b of nfft samples = x[b hop ...]: packs the overlapping blocks of an input that is only 4-byte aligned
__global__ __launch_bounds__(256) void ovsave_real_rows_kernel(const float *__restrict__ x, float *__restrict__ rows, long nblk, long nfft, long hop)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblk * nfft) return;
    const long b = i / nfft, r = i - b * nfft;
    rows[i] = x[b * hop + r];
}

static bool grid_of(long total, unsigned *g)
{
    const long n = (total + 255) / 256;
    if (n > 0x7fffffffl) return false;
    *g = (unsigned)n;
    return true;
}
hipError_t launch_ovsave_real_mul(float2 *S, const float2 *Hc, long nblk, int nbins, hipStream_t s)
{
    unsigned g;
    if (nblk <= 0) return hipSuccess;
    if (!grid_of(nblk * nbins, &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ovsave_real_mul_kernel, dim3(g), dim3(256), 0, s, S, Hc, nblk * nbins, nbins);
    return hipGetLastError();
}
hipError_t launch_ovsave_real_conj(float2 *H, int nbins, hipStream_t s)
{
    hipLaunchKernelGGL(ovsave_real_conj_kernel, dim3((unsigned)((nbins + 255) / 256)), dim3(256), 0, s, H, nbins);
    return hipGetLastError();
}
hipError_t launch_ovsave_real_scale_out(const float *y, float *out, long nblk, long nfft, long hop, float scale, hipStream_t s)
{
    unsigned g;
    if (nblk <= 0) return hipSuccess;
    if (!grid_of(nblk * (hop / 2), &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ovsave_real_scale_out_kernel, dim3(g), dim3(256), 0, s, (const float2 *)y, (float2 *)out, nblk, nfft / 2, hop / 2, scale);
    return hipGetLastError();
}
hipError_t launch_ovsave_real_rows(const float *x, float *rows, long nblk, long nfft, long hop, hipStream_t s)
{
    unsigned g;
    if (nblk <= 0) return hipSuccess;
    if (!grid_of(nblk * nfft, &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ovsave_real_rows_kernel, dim3(g), dim3(256), 0, s, x, rows, nblk, nfft, hop);
    return hipGetLastError();
}

} // namespace redio
