// fft_ct.h -- the compile-time mixed-radix family (device code and its launcher template; declared in redio_internal.h).  Two
// translation units instantiate launch_fft_ct<N> explicitly, one half of the size list each (fft_route.h: REDIO_FFT_CT_SIZES_LO / _HI
// -> fft_ct_lo.hip / fft_ct_hi.hip); the dispatcher (fft_kernels.hip: launch_fft) only sees the declaration.
#pragma once
#include "redio_internal.h"
#include "fft_wave.h"

namespace redio {

// ---- every 2^a 3^b 5^c size up to 8192 without a kernel of its own (the sizes kiss_fft_next_fast_size returns; see the
// dispatch list): the same scheme with a compile-time factor list ----
// kissfft's factor order (4s, then 2, then 3, 5; fft_plan_stages) evaluated at compile time; radix-4 neighbours run
// as register pairs -- as do any two neighbours of up to 25 points (3x2, 5x5, 5x2, 5x4 ...) -- and a stage left
// over as one pass over padded LDS; 4096 / N (at least one) transforms per
// workgroup.  Butterflies, twiddle indices and stage order are the table-driven kernel's, so results are the same bits.
template <int N>
struct FftCt {
    static constexpr int isqrt() { int r = 0; while ((r + 1) * (r + 1) <= N) ++r; return r; }
    static constexpr int MAXS = 16;
    struct List { int n; int p[MAXS], m[MAXS], fs[MAXS]; };
    static constexpr List make()
    {
        List l{};
        int p = 4, n = N, fstride = 1;
        const int fsq = isqrt();
        do {
            while (n % p) {
                switch (p) {
                case 4: p = 2; break;
                case 2: p = 3; break;
                default: p += 2; break;
                }
                if (p > fsq) p = n;
            }
            n /= p;
            l.p[l.n] = p; l.m[l.n] = n; l.fs[l.n] = fstride;
            fstride *= p;
            ++l.n;
        } while (n > 1);
        return l;
    }
    static constexpr List L = make();
    static constexpr int T = N >= 4096 ? 1 : 4096 / N;
    static constexpr int E = T * N;
    static constexpr int LDS_ELEMS = E + (E >> 3) + 8;
    __device__ static __forceinline__ int phys(int e) { return e + (e >> 3); }
    __device__ static __forceinline__ int leaf_pos(int n)
    {
        int P = 0;
#pragma unroll
        for (int s = 0; s < L.n; ++s) P += ((n / L.fs[s]) % L.p[s]) * L.m[s];
        return P;
    }
    static constexpr bool supported()
    {
        for (int s = 0; s < L.n; ++s)
            if (L.p[s] > 5) return false;
        return true;
    }
    // the stage-ordered twiddle copy of the plan (redio_api.hip): stage s holds T[toff(s) + (n - 1) m + k] = tw[n k fstride],
    // n = 1 .. p - 1, k < m, so lanes with neighbouring k read neighbouring entries
    static constexpr int toff(int s)
    {
        int o = 0;
        for (int u = 0; u < s; ++u) o += (L.p[u] - 1) * L.m[u];
        return o;
    }
};

struct CtView { // one transform inside the padded batch image
    float2 *p; int off;
    __device__ __forceinline__ float2 &operator[](int i) const { const int e = off + i; return p[e + (e >> 3)]; }
};

// one radix-P butterfly on P contiguous register values: index k inside the sub-length m, twiddle stride fs
// (the argument lists of fft_stage_butterfly_gk)
template <int P, bool INV>
__device__ __forceinline__ void fftct_bfly(float2 (&a)[P], const float2 *__restrict__ Ts, const float2 *__restrict__ tw, int k, int fs, int m)
{
    if constexpr (P == 2) bfly2(a[0], a[1], Ts[k]);
    else if constexpr (P == 3) bfly3(a[0], a[1], a[2], Ts[k], Ts[m + k], tw[fs * m]);
    else if constexpr (P == 4) bfly4<INV>(a[0], a[1], a[2], a[3], Ts[k], Ts[m + k], Ts[2 * m + k]);
    else bfly5(a[0], a[1], a[2], a[3], a[4], Ts[k], Ts[m + k], Ts[2 * m + k], Ts[3 * m + k], tw[fs * m], tw[fs * 2 * m]);
}

template <int NTH>
__device__ __forceinline__ void fftct_sync()
{
    if constexpr (NTH == 64) wave_lds_fence(); // the image belongs to one wave: LDS operations of a wave complete in order
    else __syncthreads();
}

template <int N, bool INV, int S, int NTH = 256, int EPTS = FftCt<N>::E>
__device__ __forceinline__ void fftct_stages(float2 *Ls, const float2 *__restrict__ tw, const float2 *__restrict__ T, int tid)
{
    using F = FftCt<N>;
    if constexpr (S >= 0) {
        constexpr int P = F::L.p[S], M = F::L.m[S], FS = F::L.fs[S];
        constexpr int PO = S >= 1 ? F::L.p[S >= 1 ? S - 1 : 0] : 0; // the next stage out
        if constexpr (S >= 1 && P * PO <= 25) {
            // two stages in registers: P*PO points base + j*M; inner radix P (sub-length M), outer radix PO (sub-length P*M)
            constexpr int FS2 = F::L.fs[S - 1], G = P * PO;
#pragma unroll 1
            for (int g = tid; g < EPTS / G; g += NTH) {
                const int xf = g / (N / G), gl = g % (N / G);
                const int blk = gl / M, kk = gl % M;
                const int base = xf * N + blk * G * M + kk;
                float2 a[G];
#pragma unroll
                for (int j = 0; j < G; ++j) a[j] = Ls[F::phys(base + j * M)];
#pragma unroll
                for (int q = 0; q < PO; ++q) {
                    float2 b[P];
#pragma unroll
                    for (int i = 0; i < P; ++i) b[i] = a[q * P + i];
                    fftct_bfly<P, INV>(b, T + F::toff(S), tw, kk, FS, M);
#pragma unroll
                    for (int i = 0; i < P; ++i) a[q * P + i] = b[i];
                }
#pragma unroll
                for (int u = 0; u < P; ++u) {
                    float2 b[PO];
#pragma unroll
                    for (int i = 0; i < PO; ++i) b[i] = a[u + P * i];
                    fftct_bfly<PO, INV>(b, T + F::toff(S - 1), tw, kk + u * M, FS2, P * M);
#pragma unroll
                    for (int i = 0; i < PO; ++i) a[u + P * i] = b[i];
                }
#pragma unroll
                for (int j = 0; j < G; ++j) Ls[F::phys(base + j * M)] = a[j];
            }
            fftct_sync<NTH>();
            fftct_stages<N, INV, S - 2, NTH, EPTS>(Ls, tw, T, tid);
        } else {
#pragma unroll 1
            for (int bb = tid; bb < EPTS / P; bb += NTH) {
                const int xf = bb / (N / P), b = bb % (N / P);
                const int base = xf * N + (b / M) * P * M + (b % M);
                float2 a[P];
#pragma unroll
                for (int j = 0; j < P; ++j) a[j] = Ls[F::phys(base + j * M)];
                fftct_bfly<P, INV>(a, T + F::toff(S), tw, b % M, FS, M);
#pragma unroll
                for (int j = 0; j < P; ++j) Ls[F::phys(base + j * M)] = a[j];
            }
            fftct_sync<NTH>();
            fftct_stages<N, INV, S - 1, NTH, EPTS>(Ls, tw, T, tid);
        }
    }
}

// 600 ... 1280 points (launch_fft_ct): every wave owns its own transforms (about 1024 points, at least one transform) in its
// own LDS image, so the passes are separated by compiler fences instead of workgroup barriers
template <int N>
struct FftCtW {
    static constexpr int TW = N >= 1024 ? 1 : 1024 / N;      // transforms per wave
    static constexpr int EW = TW * N;
    static constexpr int LDS_W = (EW + (EW >> 3) + 8 + 1) & ~1; // float2 per wave
};
template <int N, bool INV>
__global__ __launch_bounds__(256) void fft_ct_wave_kernel(const float2 *in, float2 *out, const float2 *__restrict__ tw, const float2 *__restrict__ T, long nbatch, long in_stride)
{
    using F = FftCt<N>;
    using W = FftCtW<N>;
    static_assert(F::supported(), "radices up to 5 only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float2 *Ls = reinterpret_cast<float2 *>(smem) + w * W::LDS_W;
    const long b0 = ((long)blockIdx.x * 4 + w) * W::TW;
    if (b0 >= nbatch) return; // wave-uniform; no workgroup barrier in this kernel
#pragma unroll 4
    for (int e = lane; e < W::EW; e += 64) {
        const int xf = e / N, n = e % N;
        const long b = (b0 + xf < nbatch) ? b0 + xf : nbatch - 1;
        Ls[F::phys(xf * N + F::leaf_pos(n))] = in[b * in_stride + n];
    }
    wave_lds_fence();
    fftct_stages<N, INV, F::L.n - 1, 64, W::EW>(Ls, tw, T, lane);
#pragma unroll 4
    for (int e = lane; e < W::EW; e += 64) {
        const int xf = e / N;
        if (b0 + xf < nbatch) out[(b0 + xf) * N + (e % N)] = Ls[F::phys(e)];
    }
}

template <int N, bool INV>
__global__ __launch_bounds__(256) void fft_ct_kernel(const float2 *in, float2 *out, const float2 *__restrict__ tw, const float2 *__restrict__ T, long nbatch, long in_stride)
{
    using F = FftCt<N>;
    static_assert(F::supported(), "radices up to 5 only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *Ls = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    const long b0 = (long)blockIdx.x * F::T;
#pragma unroll 4
    for (int e = tid; e < F::E; e += 256) {
        const int xf = e / N, n = e % N;
        const long b = (b0 + xf < nbatch) ? b0 + xf : nbatch - 1;
        Ls[F::phys(xf * N + F::leaf_pos(n))] = in[b * in_stride + n];
    }
    __syncthreads();
    fftct_stages<N, INV, F::L.n - 1>(Ls, tw, T, tid);
#pragma unroll 4
    for (int e = tid; e < F::E; e += 256) {
        const int xf = e / N;
        if (b0 + xf < nbatch) out[(b0 + xf) * N + (e % N)] = Ls[F::phys(e)];
    }
}

// one transform per NTH-thread workgroup: 1281 ... 2048 points with 128 threads (two waves meet at the barriers instead of
// four), more than 5120 points with 512 (more waves to hide the LDS round trips of a 50-70 KiB image)
template <int N, bool INV, int NTH = 128>
__global__ __launch_bounds__(NTH) void fft_ct_pair_kernel(const float2 *in, float2 *out, const float2 *__restrict__ tw, const float2 *__restrict__ T, long in_stride)
{
    using F = FftCt<N>;
    static_assert(F::supported(), "radices up to 5 only");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *Ls = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x;
    const float2 *src = in + (long)blockIdx.x * in_stride;
#pragma unroll 4
    for (int n = tid; n < N; n += NTH) Ls[F::phys(F::leaf_pos(n))] = src[n];
    __syncthreads();
    fftct_stages<N, INV, F::L.n - 1, NTH, N>(Ls, tw, T, tid);
    float2 *dst = out + (long)blockIdx.x * N;
#pragma unroll 4
    for (int n = tid; n < N; n += NTH) dst[n] = Ls[F::phys(n)];
}

template <int N>
hipError_t launch_fft_ct(const FftPlanDev &p, const float2 *in, float2 *out, long nbatch, long in_stride, bool inv, hipStream_t s)
{
    using F = FftCt<N>;
    // the compile-time list must be the plan's (it is the same algorithm; a mismatch would mean a different build)
    if (p.nstages != F::L.n || !p.tw_pass) return hipErrorNotSupported;
    for (int i = 0; i < F::L.n; ++i)
        if (p.st[i].p != F::L.p[i] || p.st[i].m != F::L.m[i] || p.st[i].fstride != F::L.fs[i]) return hipErrorNotSupported;
    // measured per size: one transform (or a few) per wave wins from 600 to 1280 points (+2 ... +21 %) and at 384 (+13 %);
    // smaller sizes leave lanes idle in the 16-point passes, larger ones take too much LDS per workgroup
    if constexpr ((N >= 600 && N <= 1280) || N == 384) {
        using W = FftCtW<N>;
        const size_t ldsw = (size_t)4 * W::LDS_W * sizeof(float2);
        auto wf = fft_ct_wave_kernel<N, false>;
        auto wi = fft_ct_wave_kernel<N, true>;
        if (ldsw > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(inv ? wi : wf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsw);
            if (e != hipSuccess) return e;
        }
        const long nwaves = (nbatch + W::TW - 1) / W::TW;
        const unsigned gridw = (unsigned)((nwaves + 3) / 4);
        if (inv) hipLaunchKernelGGL(wi, dim3(gridw), dim3(256), ldsw, s, in, out, p.tw, p.tw_pass, nbatch, in_stride);
        else hipLaunchKernelGGL(wf, dim3(gridw), dim3(256), ldsw, s, in, out, p.tw, p.tw_pass, nbatch, in_stride);
        return hipGetLastError();
    } else if constexpr (N > 1280 && N <= 2048) { // measured +9 ... +18 % over two transforms per 256-thread workgroup; slower above 2048
        const size_t ldsp = (size_t)(N + (N >> 3) + 8) * sizeof(float2);
        if (inv) hipLaunchKernelGGL((fft_ct_pair_kernel<N, true>), dim3((unsigned)nbatch), dim3(128), ldsp, s, in, out, p.tw, p.tw_pass, in_stride);
        else hipLaunchKernelGGL((fft_ct_pair_kernel<N, false>), dim3((unsigned)nbatch), dim3(128), ldsp, s, in, out, p.tw, p.tw_pass, in_stride);
        return hipGetLastError();
    } else if constexpr (N > 8192) { // 8193 ... 16384 points: the image takes most of a CU's LDS; sixteen waves on it
        const size_t ldsp = (size_t)(N + (N >> 3) + 8) * sizeof(float2);
        auto kf10 = fft_ct_pair_kernel<N, false, 1024>;
        auto ki10 = fft_ct_pair_kernel<N, true, 1024>;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(inv ? ki10 : kf10), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsp);
        if (e != hipSuccess) return e;
        if (inv) hipLaunchKernelGGL(ki10, dim3((unsigned)nbatch), dim3(1024), ldsp, s, in, out, p.tw, p.tw_pass, in_stride);
        else hipLaunchKernelGGL(kf10, dim3((unsigned)nbatch), dim3(1024), ldsp, s, in, out, p.tw, p.tw_pass, in_stride);
        return hipGetLastError();
    } else if constexpr (N > 5120) { // eight waves on one transform: measured +10 ... +26 % over four (5120 itself is faster with four)
        const size_t ldsp = (size_t)(N + (N >> 3) + 8) * sizeof(float2);
        auto kf5 = fft_ct_pair_kernel<N, false, 512>;
        auto ki5 = fft_ct_pair_kernel<N, true, 512>;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(inv ? ki5 : kf5), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ldsp);
        if (e != hipSuccess) return e;
        if (inv) hipLaunchKernelGGL(ki5, dim3((unsigned)nbatch), dim3(512), ldsp, s, in, out, p.tw, p.tw_pass, in_stride);
        else hipLaunchKernelGGL(kf5, dim3((unsigned)nbatch), dim3(512), ldsp, s, in, out, p.tw, p.tw_pass, in_stride);
        return hipGetLastError();
    } else {
        const size_t lds = (size_t)F::LDS_ELEMS * sizeof(float2);
        auto kf = fft_ct_kernel<N, false>;
        auto ki = fft_ct_kernel<N, true>;
        if (lds > 48 * 1024) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(inv ? ki : kf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            if (e != hipSuccess) return e;
        }
        const unsigned grid = (unsigned)((nbatch + F::T - 1) / F::T);
        if (inv) hipLaunchKernelGGL(ki, dim3(grid), dim3(256), lds, s, in, out, p.tw, p.tw_pass, nbatch, in_stride);
        else hipLaunchKernelGGL(kf, dim3(grid), dim3(256), lds, s, in, out, p.tw, p.tw_pass, nbatch, in_stride);
        return hipGetLastError();
    }
}

} // namespace redio
