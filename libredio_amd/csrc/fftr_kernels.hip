// fftr_kernels.hip -- gfx950 kernels of the real-input transform (kiss_fftr / kiss_fftri; arithmetic: fftr_core.h).
//
// Bound: HBM.  Two strategies:
//   fftr1k_fwd_kernel / fftr1k_inv_kernel   N = 2048 real points (M = 1024): the one-wavefront transform of fft_wave.h with the split
//                       step fused in -- forward through the wave's own LDS image, inverse ahead of the first pass.  One read of
//                       the real row and one write of the M + 1 bins (or the reverse): 8 B per real sample.
//   fftr_post_kernel / fftr_pre_kernel      every other even N: the split as its own pass next to the complex plan of size M
//                       (plan-owned scratch in between): 16 B per real sample.
#include "redio_internal.h"
#include "fft_wave.h"
#include "fftr_core.h"

namespace redio {

// One wavefront per transform, FFT1K_RUN consecutive transforms per wavefront, the next row's loads issued under this row's
// arithmetic (the schedule of fft1k_wave_kernel).  Spectrum rows are only 8-byte aligned (M + 1 = 1025 cf32): every access on that
// side is one float2.
constexpr int FFTR1K_RUN = 4;

__global__ __launch_bounds__(256) void fftr1k_fwd_kernel(const float *in, float2 *out, const float2 *__restrict__ tw,
                                                         const float2 *__restrict__ stw, long nbatch, long in_stride, long out_stride)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *ex = reinterpret_cast<float2 *>(smem) + wave * FFT1K_LDS;
    const long b0 = ((long)blockIdx.x * 4 + wave) * FFTR1K_RUN;
    if (b0 >= nbatch) return; // wave-uniform
    const long b1 = (b0 + FFTR1K_RUN < nbatch) ? b0 + FFTR1K_RUN : nbatch;
    Fft1kTw t;
    fft1k_load_tw(t, lane, tw);
    Fftr1kTw w;
    fftr1k_load_tw(w, lane, stw);
    float2 v[16], nx[16];
    {
        const float2 *row = reinterpret_cast<const float2 *>(in + b0 * in_stride); // the real row as M cf32
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = row[lane + 64 * i];
    }
    for (long b = b0; b < b1; ++b) {
        const long bn = (b + 1 < b1) ? b + 1 : b;
        const float2 *row = reinterpret_cast<const float2 *>(in + bn * in_stride);
#pragma unroll
        for (int i = 0; i < 16; ++i) nx[i] = row[lane + 64 * i];
        fft1k_wave_stages0to3<false>(v, ex, tw, t, lane);
        fft1k_passC<false>(v, t);
        wave_lds_fence(); // every lane has read its last-stage inputs before Z overwrites the image
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) ex[lane + 64 * q + 256 * j] = v[4 * q + j];
        wave_lds_fence();
        fftr1k_post_lane(v, ex, w, lane, out + b * out_stride);
        wave_lds_fence();
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = nx[i];
    }
}

__global__ __launch_bounds__(256) void fftr1k_inv_kernel(const float2 *in, float *out, const float2 *__restrict__ tw,
                                                         const float2 *__restrict__ stw, long nbatch, long in_stride, long out_stride)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *ex = reinterpret_cast<float2 *>(smem) + wave * FFT1K_LDS;
    const long b0 = ((long)blockIdx.x * 4 + wave) * FFTR1K_RUN;
    if (b0 >= nbatch) return; // wave-uniform
    const long b1 = (b0 + FFTR1K_RUN < nbatch) ? b0 + FFTR1K_RUN : nbatch;
    Fft1kTw t;
    fft1k_load_tw(t, lane, tw);
    Fftr1kTw w;
    fftr1k_load_tw(w, lane, stw);
    float2 a[8], c[8], mid, v[16];
    fftr1k_load_row(in + b0 * in_stride, lane, a, c, mid);
    for (long b = b0; b < b1; ++b) {
        fftr1k_pre_lane(a, c, mid, w, lane, v, ex);
        wave_lds_fence();
        fftr1k_pre_gather(v, ex, lane);
        const long bn = (b + 1 < b1) ? b + 1 : b; // the next row's bins travel under this row's transform
        fftr1k_load_row(in + bn * in_stride, lane, a, c, mid);
        fft1k_wave_regs<true>(v, reinterpret_cast<float2 *>(out + b * out_stride), ex, tw, t, lane);
        wave_lds_fence();
    }
}

// ---- every other size: thread (row, j), j = 0 ... M / 2.  A block of 256 threads holds 256 >> lgW rows of W = 1 << lgW steps
// (W: the power of two at or above M / 2 + 1, 256 at most; beyond that blockIdx.y counts 256-step pieces of one row), so one
// geometry serves M = 1 as well as M = 65536.  Z[j] is read in ascending, Z[M - j] in descending order: both coalesced.
__global__ __launch_bounds__(256) void fftr_post_kernel(const float2 *__restrict__ z, long z_stride, float2 *__restrict__ f, long f_stride,
                                                        const float2 *__restrict__ stw, int M, long nbatch, int lgW)
{
    const long row = (long)blockIdx.x * (256 >> lgW) + (threadIdx.x >> lgW);
    const int j = (int)blockIdx.y * 256 + (int)(threadIdx.x & ((1u << lgW) - 1));
    if (row >= nbatch || j > M / 2) return;
    fftr_post_thread(j, M, z + row * z_stride, f + row * f_stride, stw);
}
__global__ __launch_bounds__(256) void fftr_pre_kernel(const float2 *__restrict__ f, long f_stride, float2 *__restrict__ t, long t_stride,
                                                       const float2 *__restrict__ stw, int M, long nbatch, int lgW)
{
    const long row = (long)blockIdx.x * (256 >> lgW) + (threadIdx.x >> lgW);
    const int j = (int)blockIdx.y * 256 + (int)(threadIdx.x & ((1u << lgW) - 1));
    if (row >= nbatch || j > M / 2) return;
    fftr_pre_thread(j, M, f + row * f_stride, t + row * t_stride, stw);
}

hipError_t launch_fftr1k(bool inverse, const void *in, void *out, const float2 *tw, const float2 *stw, long nbatch, long in_stride,
                         long out_stride, hipStream_t s)
{
    if (nbatch <= 0) return hipSuccess;
    const size_t lds = 4 * FFT1K_LDS * sizeof(float2);
    const unsigned grid = (unsigned)((nbatch + 4 * FFTR1K_RUN - 1) / (4 * FFTR1K_RUN));
    if (inverse)
        hipLaunchKernelGGL(fftr1k_inv_kernel, dim3(grid), dim3(256), lds, s, (const float2 *)in, (float *)out, tw, stw, nbatch, in_stride, out_stride);
    else
        hipLaunchKernelGGL(fftr1k_fwd_kernel, dim3(grid), dim3(256), lds, s, (const float *)in, (float2 *)out, tw, stw, nbatch, in_stride, out_stride);
    return hipGetLastError();
}

hipError_t launch_fftr_split(bool inverse, const float2 *src, long src_stride, float2 *dst, long dst_stride, const float2 *stw, int M, long nbatch,
                             hipStream_t s)
{
    if (nbatch <= 0) return hipSuccess;
    const int per = M / 2 + 1;
    int lgW = 0;
    while (lgW < 8 && (1 << lgW) < per) ++lgW;
    const long rows = 256 >> lgW;
    const long gx = (nbatch + rows - 1) / rows;
    if (gx > 0x7fffffffl) return hipErrorInvalidValue;
    const dim3 grid((unsigned)gx, (unsigned)((per + 255) / 256));
    if (inverse) hipLaunchKernelGGL(fftr_pre_kernel, grid, dim3(256), 0, s, src, src_stride, dst, dst_stride, stw, M, nbatch, lgW);
    else hipLaunchKernelGGL(fftr_post_kernel, grid, dim3(256), 0, s, src, src_stride, dst, dst_stride, stw, M, nbatch, lgW);
    return hipGetLastError();
}

} // namespace redio
