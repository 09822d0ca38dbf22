// pspec_kernels.hip -- gfx950 kernels of the integrated power spectrum (redio_pspec_*; contract: DESIGN.md 5.3c).
//
// Bound: HBM.  Two strategies:
//   pspec1k_kernel        N = 1024: one wavefront per unit (a whole row of K transforms, or one segment of at most 16) runs the
//                         one-wave transform of fft_wave.h on each transform and squares and accumulates its result registers; the
//                         spectra never leave the wave.  8 N / step bytes read and 4 / K written per sample.
//   the small kernels below  every other N: the row gather (window, overlap), the accumulate pass over the plan's own redio_fft
//                         spectra and the fold of the segment partials (pspec_api.hip).  The fold also ends the fused kernel's
//                         segment mode.
//   pspec1k_u8_kernel, pspec_rows_u8_kernel  the two entry kernels fed with the receiver's u8 I/Q bytes (redio_pspec_enqueue_u8):
//                         2 N / step bytes read per sample; the conversion is part of the load.
#include "redio_internal.h"
#include "fft_wave.h"
#include "pspec_core.h"

namespace redio {

// One wavefront per unit, four per workgroup; the next transform's samples are loaded under this one's arithmetic (the schedule of
// fft1k_wave_kernel).  dst: unit u's 1024 f32 at dst + 1024 u (the output rows, or the segment partials when `split`).
template <bool WIN>
__global__ __launch_bounds__(256) void pspec1k_kernel(const float2 *__restrict__ x, long step, long K, const float *__restrict__ win,
                                                      const float2 *__restrict__ tw, float *__restrict__ dst, long nunits, int split)
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
    float w[16];
    if (WIN) pspec1k_load_window(w, win, lane);
    float2 v[16], nx[16];
    float seg[16], row[16];
    const float2 *p = x + g0 * step;
    pspec1k_load(v, p, lane);
    for (long i = 0; i < cnt; ++i) {
        const float2 *pn = (i + 1 < cnt) ? p + step : p; // prefetch the next transform's input under this one's arithmetic
        pspec1k_load(nx, pn, lane);
        if (WIN) pspec1k_window(v, w);
        fft1k_wave_stages0to3<false>(v, ex, tw, t, lane);
        fft1k_passC<false>(v, t);
        const PspecStep s = pspec_step(i, cnt); // wave-uniform
        pspec1k_accum(v, seg, s.seg_first);
        if (s.seg_last) pspec1k_fold(seg, row, s.row_first);
        wave_lds_fence();
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = nx[e];
        p = pn;
    }
    pspec1k_store(row, dst + u * 1024, lane);
}

hipError_t launch_pspec1k(const float2 *x, long step, long K, const float *win, const float2 *tw, float *dst, long nunits, bool split, hipStream_t s)
{
    if (nunits <= 0) return hipSuccess;
    const size_t lds = 4 * FFT1K_LDS * sizeof(float2);
    const long g = (nunits + 3) / 4;
    if (g > 0x7fffffffl) return hipErrorInvalidValue;
    if (win) hipLaunchKernelGGL(pspec1k_kernel<true>, dim3((unsigned)g), dim3(256), lds, s, x, step, K, win, tw, dst, nunits, split ? 1 : 0);
    else hipLaunchKernelGGL(pspec1k_kernel<false>, dim3((unsigned)g), dim3(256), lds, s, x, step, K, win, tw, dst, nunits, split ? 1 : 0);
    return hipGetLastError();
}

// The same kernel fed with the receiver's u8 I/Q bytes (x: one 16-bit word per sample; only 2-byte alignment is assumed).  Sixteen
// wave-wide 16-bit loads per transform, as many as the cf32 kernel's at a quarter of the bytes; the next transform is prefetched as
// raw words (16 VGPRs instead of 32) and converted (i2f) after the swap.  From the window multiply on it is pspec1k_kernel.  A
// sibling and not a template parameter: the cf32 instantiations keep their names and code.
template <bool WIN>
__global__ __launch_bounds__(256) void pspec1k_u8_kernel(const uint16_t *__restrict__ x, long step, long K, const float *__restrict__ win,
                                                         const float2 *__restrict__ tw, float *__restrict__ dst, long nunits, int split)
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
    float w[16];
    if (WIN) pspec1k_load_window(w, win, lane);
    uint16_t raw[16];
    float2 v[16];
    float seg[16], row[16];
    const uint16_t *p = x + g0 * step;
    pspec1k_load_raw(raw, p, lane);
    for (long i = 0; i < cnt; ++i) {
        pspec1k_convert(v, raw);
        // prefetch the next transform's words under this one's arithmetic.  The unit's last transform reloads its own words, as the
        // cf32 kernel does: loading only when i + 1 < cnt was measured and lost 6 % at K = 16, windowed, step 512
        const uint16_t *pn = (i + 1 < cnt) ? p + step : p;
        pspec1k_load_raw(raw, pn, lane);
        if (WIN) pspec1k_window(v, w);
        fft1k_wave_stages0to3<false>(v, ex, tw, t, lane);
        fft1k_passC<false>(v, t);
        const PspecStep s = pspec_step(i, cnt); // wave-uniform
        pspec1k_accum(v, seg, s.seg_first);
        if (s.seg_last) pspec1k_fold(seg, row, s.row_first);
        wave_lds_fence();
        p = pn;
    }
    pspec1k_store(row, dst + u * 1024, lane);
}

hipError_t launch_pspec1k_u8(const uint16_t *x, long step, long K, const float *win, const float2 *tw, float *dst, long nunits, bool split, hipStream_t s)
{
    if (nunits <= 0) return hipSuccess;
    const size_t lds = 4 * FFT1K_LDS * sizeof(float2);
    const long g = (nunits + 3) / 4;
    if (g > 0x7fffffffl) return hipErrorInvalidValue;
    if (win) hipLaunchKernelGGL(pspec1k_u8_kernel<true>, dim3((unsigned)g), dim3(256), lds, s, x, step, K, win, tw, dst, nunits, split ? 1 : 0);
    else hipLaunchKernelGGL(pspec1k_u8_kernel<false>, dim3((unsigned)g), dim3(256), lds, s, x, step, K, win, tw, dst, nunits, split ? 1 : 0);
    return hipGetLastError();
}

// ---- every other size ----------------------------------------------------------------------------
// row b of N samples = x[b step ...], times the window when there is one
__global__ __launch_bounds__(256) void pspec_rows_kernel(const float2 *__restrict__ x, const float *__restrict__ win, float2 *__restrict__ rows,
                                                         long ntr, long N, long step)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ntr * N) return;
    const long b = i / N, n = i - b * N;
    float2 v = x[b * step + n];
    if (win) {
        const float wn = win[n];
        v = make_float2(mul_rn(v.x, wn), mul_rn(v.y, wn));
    }
    rows[i] = v;
}
// the same from u8 I/Q bytes (x: one 16-bit word per sample): the conversion happens in the gather, there is no whole-message cf32 buffer.
// Two consecutive elements per lane step (two 2-byte loads, one 16-byte store: 1 KiB contiguous per wave instruction), four steps per
// thread, as data_to_samples_kernel (ingest.hip) found best; total = ntr N elements (below 2^32), rows 16-byte aligned.
__global__ __launch_bounds__(256) void pspec_rows_u8_kernel(const uint16_t *__restrict__ x, const float *__restrict__ win, float2 *__restrict__ rows,
                                                            unsigned total, unsigned N, long step)
{
    const unsigned npair = total / 2;
    unsigned q = blockIdx.x * 1024u + threadIdx.x;
#pragma unroll
    for (int j = 0; j < 4; ++j, q += 256) {
        if (q >= npair) break;
        float2 v0, v1;
        pspec_rows_u8_pair(x, win, win != nullptr, q, N, step, v0, v1);
        reinterpret_cast<float4 *>(rows)[q] = make_float4(v0.x, v0.y, v1.x, v1.y);
    }
    if ((total & 1) && blockIdx.x == 0 && threadIdx.x == 0) { // an odd count: the last element on its own
        const unsigned i = total - 1, b = i / N;
        rows[i] = pspec_rows_u8_thread(x, win, win != nullptr, (long)b, (long)(i - b * N), step);
    }
}
// one thread per segment and bin, consecutive threads on consecutive bins; spec: the spectrum of transform g_base (counted from the
// call's first); segments q0 ... q0 + nseg - 1; dst: N f32 per segment of the CALL (the partials, or the rows when K <= 16)
__global__ __launch_bounds__(256) void pspec_accum_kernel(const float2 *__restrict__ spec, float *__restrict__ dst, long q0, long nseg, long N,
                                                          long K, long S, long g_base)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nseg * N) return;
    const long qi = i / N, k = i - qi * N;
    long g, cnt;
    pspec_segment(q0 + qi, K, S, g, cnt);
    dst[(q0 + qi) * N + k] = pspec_accum_thread(spec + (g - g_base) * N, N, cnt, k);
}
// one thread per row and bin
__global__ __launch_bounds__(256) void pspec_fold_kernel(const float *__restrict__ part, float *__restrict__ out, long nrows, long N, long S)
{
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nrows * N) return;
    const long r = i / N, k = i - r * N;
    out[i] = pspec_fold_thread(part + r * S * N, N, S, k);
}

static bool grid_of(long total, unsigned *g)
{
    const long n = (total + 255) / 256;
    if (n > 0x7fffffffl) return false;
    *g = (unsigned)n;
    return true;
}
hipError_t launch_pspec_rows(const float2 *x, const float *win, float2 *rows, long ntr, long N, long step, hipStream_t s)
{
    unsigned g;
    if (ntr <= 0) return hipSuccess;
    if (!grid_of(ntr * N, &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pspec_rows_kernel, dim3(g), dim3(256), 0, s, x, win, rows, ntr, N, step);
    return hipGetLastError();
}
hipError_t launch_pspec_rows_u8(const uint16_t *x, const float *win, float2 *rows, long ntr, long N, long step, hipStream_t s)
{
    if (ntr <= 0) return hipSuccess;
    const long total = ntr * N; // a chunk: at most 64 MiB of rows, or one segment
    if (total >= (1l << 32)) return hipErrorInvalidValue;
    const long g = (total / 2 + 1023) / 1024;
    hipLaunchKernelGGL(pspec_rows_u8_kernel, dim3((unsigned)(g < 1 ? 1 : g)), dim3(256), 0, s, x, win, rows, (unsigned)total, (unsigned)N, step);
    return hipGetLastError();
}
hipError_t launch_pspec_accum(const float2 *spec, float *dst, long q0, long nseg, long N, long K, long g_base, hipStream_t s)
{
    unsigned g;
    if (nseg <= 0) return hipSuccess;
    if (!grid_of(nseg * N, &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pspec_accum_kernel, dim3(g), dim3(256), 0, s, spec, dst, q0, nseg, N, K, pspec_nseg(K), g_base);
    return hipGetLastError();
}
hipError_t launch_pspec_fold(const float *part, float *out, long nrows, long N, long S, hipStream_t s)
{
    unsigned g;
    if (nrows <= 0) return hipSuccess;
    if (!grid_of(nrows * N, &g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pspec_fold_kernel, dim3(g), dim3(256), 0, s, part, out, nrows, N, S);
    return hipGetLastError();
}

} // namespace redio
