// pspec_real_kernels.hip -- gfx950 kernels of the real-input integrated power spectrum (redio_pspec_real_*; contract: DESIGN.md 5.3d).
//
// Bound: HBM.  Two strategies:
//   pspecr2k_kernel         N = 2048 real points (M = 1024): one wavefront per unit (a whole row of K transforms, or one segment of at
//                           most 16) runs the one-wave transform of fft_wave.h on the row read as M cf32, the split step of
//                           fftr_core.h through the wave's own LDS image, and squares and accumulates the 1025 bins in registers; the
//                           spectra never leave the wave.  4 N / step bytes read and about 2 / K written per real sample.
//   pspec_real_rows_kernel  every other even N: the row gather (window, overlap, 4-byte aligned streams) ahead of the plan's own
//                           redio_fftr; the accumulate and fold passes are pspec_kernels.hip's with a row of N / 2 + 1 bins
//                           (pspec_api.hip).  The fold also ends the fused kernel's segment mode.
#include "redio_internal.h"
#include "fft_wave.h"
#include "pspec_real_core.h"

namespace redio {

// One wavefront per unit, four per workgroup; the next transform's samples are loaded under this one's arithmetic (the schedule of
// pspec1k_kernel).  dst: unit u's 1025 f32 at dst + 1025 u (the output rows, or the segment partials when `split`).  PAIRS: every
// transform of the call starts on an 8-byte boundary (the host checks the base address and that step is even).  A sibling of
// pspec1k_kernel and fftr1k_fwd_kernel, not a template parameter on them: they keep their names and code.
template <bool WIN, bool PAIRS>
__global__ __launch_bounds__(256) void pspecr2k_kernel(const float *__restrict__ x, long step, long K, const float *__restrict__ win,
                                                       const float2 *__restrict__ tw, const float2 *__restrict__ stw, float *__restrict__ dst,
                                                       long nunits, int split)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *ex = reinterpret_cast<float2 *>(smem) + wave * FFT1K_LDS;
    const long u = (long)blockIdx.x * 4 + wave;
    if (u >= nunits) return; // wave-uniform
    long g0, cnt;
    pspec_unit(u, K, split != 0, g0, cnt);
    Fft1kTw t;
    fft1k_load_tw(t, lane, tw);
    Fftr1kTw sw;
    fftr1k_load_tw(sw, lane, stw);
    float2 w[16];
    if (WIN) pspecr2k_load_window(w, win, lane);
    float2 v[16], nx[16];
    float p[17], seg[17], row[17];
    const float *q = x + g0 * step;
    if (PAIRS) pspecr2k_load_pairs(v, reinterpret_cast<const float2 *>(q), lane);
    else pspecr2k_load_singles(v, q, lane);
    for (long i = 0; i < cnt; ++i) {
        // prefetch the next transform's row under this one's arithmetic.  The unit's last transform reloads its own row, as the cf32
        // kernel does: loading only when i + 1 < cnt was measured there and lost 6 %
        const float *qn = (i + 1 < cnt) ? q + step : q;
        if (PAIRS) pspecr2k_load_pairs(nx, reinterpret_cast<const float2 *>(qn), lane);
        else pspecr2k_load_singles(nx, qn, lane);
        if (WIN) pspecr2k_window(v, w);
        fft1k_wave_stages0to3<false>(v, ex, tw, t, lane);
        fft1k_passC<false>(v, t);
        wave_lds_fence(); // every lane has read its last-stage inputs before Z overwrites the image
        pspecr2k_image(v, ex, lane);
        wave_lds_fence();
        pspecr2k_split_power(v, ex, sw, lane, p);
        const PspecStep s = pspec_step(i, cnt); // wave-uniform
        pspecr2k_accum(p, seg, s.seg_first);
        if (s.seg_last) pspecr2k_fold(seg, row, s.row_first);
        wave_lds_fence();
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = nx[e];
        q = qn;
    }
    pspecr2k_store(row, dst + u * PSPECR2K_B, lane);
}

hipError_t launch_pspecr2k(const float *x, long step, long K, const float *win, const float2 *tw, const float2 *stw, float *dst, long nunits,
                           bool split, hipStream_t s)
{
    if (nunits <= 0) return hipSuccess;
    const size_t lds = 4 * FFT1K_LDS * sizeof(float2);
    const long g = (nunits + 3) / 4;
    if (g > 0x7fffffffl) return hipErrorInvalidValue;
    const bool pairs = ((uintptr_t)x & 7) == 0 && (step & 1) == 0; // then every transform's row is 8-byte aligned
    const int sp = split ? 1 : 0;
#define PSPECR2K_GO(WIN, PAIRS) \
    hipLaunchKernelGGL((pspecr2k_kernel<WIN, PAIRS>), dim3((unsigned)g), dim3(256), lds, s, x, step, K, win, tw, stw, dst, nunits, sp)
    if (win) {
        if (pairs) PSPECR2K_GO(true, true);
        else PSPECR2K_GO(true, false);
    } else {
        if (pairs) PSPECR2K_GO(false, true);
        else PSPECR2K_GO(false, false);
    }
#undef PSPECR2K_GO
    return hipGetLastError();
}

// ---- every other size ----------------------------------------------------------------------------
// packed row b of N f32 = x[b step ...], times the window when there is one; one thread per element
__global__ __launch_bounds__(256) void pspec_real_rows_kernel(const float *__restrict__ x, const float *__restrict__ win, float *__restrict__ rows,
                                                              long ntr, long N, long step)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntr * N) return;
    const long b = i / N, n = i - b * N;
    rows[i] = pspec_real_rows_thread(x, win, win != nullptr, b, n, step);
}

hipError_t launch_pspec_real_rows(const float *x, const float *win, float *rows, long ntr, long N, long step, hipStream_t s)
{
    if (ntr <= 0) return hipSuccess;
    const long g = (ntr * N + 255) / 256;
    if (g > 0x7fffffffl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pspec_real_rows_kernel, dim3((unsigned)g), dim3(256), 0, s, x, win, rows, ntr, N, step);
    return hipGetLastError();
}

} // namespace redio
