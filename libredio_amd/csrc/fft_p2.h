// fft_p2.h -- the LDS image and the compile-time stages of the small powers of two, and the twiddle access of the compile-time
// power-of-two programs (device only): shared by fft_kernels.hip (fft_p2_kernel, the one-wave programs) and the one-kernel
// channelizer that runs the same transform on its own image (pfb_p2.hip).
#pragma once
#include "fft_core.h"

namespace redio {

// the one-wave programs (2048 and 4096 points, also as the quarters of 8192 and 16384) read their twiddles from a
// stage-ordered copy of the table: the stage with sub-length m = NS / (4 fs) starts at m - ML (ML = 1 for 4096 = 4^6,
// 2 for 2048 = 2 * 4^5) and holds T[(n - 1) m + k] = tw[n k fs] (fftbig_tables_build), so that lanes with neighbouring k
// read neighbouring entries (in table order the 64 twiddles of a wave's stage-4 load are spread over 16 to 64 cache lines)
template <int NS, int ML>
struct TwProgram { const float2 *T; };
template <int NS, int ML>
__device__ __forceinline__ float2 tw_get(TwProgram<NS, ML> p, unsigned k, unsigned fs, unsigned n)
{
    const unsigned m = NS / (4 * fs);
    return p.T[(m - ML) + (n - 1) * m + k];
}
template <typename TwPtr>
__device__ __forceinline__ float2 tw_get(TwPtr tw, unsigned k, unsigned fs, unsigned n) { return tw[n * k * fs]; }

// ---- small powers of two and N = 2 * 4^L up to 512 (2, 4, 8, 16, 32, 128, 512; 2048 and 8192 have their own kernels below): compile-time stages in LDS
// kissfft factors 2 * 4^L as 4, 4, ..., 4, 2 with the radix-2 stage innermost.  One 256-thread workgroup
// handles 4096 points (8192 for the largest size): max(1, 4096 / N) transforms.  Coalesced load with the
// digit reversal applied on the LDS side, then register passes over LDS (one pad float2 per 8 keeps the
// 8-point first pass conflict-free): [radix-2 + radix-4 on 8 consecutive positions], then pairs of radix-4
// stages on 16 points per thread, a single radix-4 stage if one is left, coalesced store.  Every index is
// a compile-time shift; butterflies, twiddle indices and stage order are kissfft's (bit-identical).
template <int LOG2N>
struct FftP2 {
    static constexpr int N = 1 << LOG2N, L4 = LOG2N / 2;
    static constexpr bool ODD = (LOG2N & 1) != 0; // a radix-2 stage innermost
    static constexpr int E = N >= 4096 ? N : 4096; // points per workgroup
    static constexpr int T = E / N;                // transforms per workgroup
    // one pad float2 per 8.  Round 6 modelled every LDS access of the kernels on this image (tools/p2_lds_model.py: 50 % of the LDS-array cycles at 256
    // points are bank conflicts, SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE measures 47 %) and tried one pad per 16 for 128 points and more, which halves
    // them in the model -- measured: 256 channels + 0.8 %, 1024 channels - 3.7 %, 512 - 1.5 %, the 128-point transform - 2.3 %
    // (profiles/r06_p2_lds_padding.txt): the LDS array is not what these kernels wait for.  Kept at 8.
    __device__ static __forceinline__ int phys(int e) { return e + (e >> 3); }
    static constexpr int LDS_ELEMS = E + (E >> 3) + 8;
    // leaf position of input index n: the top bit is the radix-2 digit, base-4 digits reverse onto N/4, N/16, ...
    __device__ static __forceinline__ int leaf_pos(int n)
    {
        int P = ODD ? n >> (2 * L4) : 0;
#pragma unroll
        for (int i = 0; i < L4; ++i) P += ((n >> (2 * i)) & 3) * (N >> (2 * i + 2));
        return P;
    }
};

// LB: the workgroup barriers between the stages order LDS traffic only and the caller keeps global requests in flight across them
// (pfb_p2_kernel): `s_waitcnt lgkmcnt(0); s_barrier` instead of __syncthreads(), whose fence also waits for those requests (vmcnt(0))
template <bool LB>
__device__ __forceinline__ void fftp2_barrier()
{
    if constexpr (LB) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
}
template <int LOG2N, bool INV, int M, typename TwPtr, bool LB = false>
__device__ __forceinline__ void fftp2_rest(float2 *Ls, TwPtr tw, int tid)
{
    using F = FftP2<LOG2N>;
    constexpr int N = F::N, E = F::E;
    if constexpr (M * 4 <= N / 4) { // two stages: sub-lengths M and 4M on 16 points base + j*M
        constexpr int FS = N / (4 * M), FS2 = N / (16 * M);
#pragma unroll 1
        for (int g = tid; g < E / 16; g += 256) {
            const int xf = g / (N / 16), gl = g % (N / 16);
            const int blk = gl / M, kk = gl % M;
            const int base = xf * N + blk * 16 * M + kk;
            float2 a[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) a[j] = Ls[F::phys(base + j * M)];
            const float2 t1 = tw_get(tw, (unsigned)kk, (unsigned)FS, 1), t2 = tw_get(tw, (unsigned)kk, (unsigned)FS, 2), t3 = tw_get(tw, (unsigned)kk, (unsigned)FS, 3);
#pragma unroll
            for (int q = 0; q < 4; ++q) bfly4<INV>(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3], t1, t2, t3);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k2 = kk + u * M;
                bfly4<INV>(a[u], a[u + 4], a[u + 8], a[u + 12], tw_get(tw, (unsigned)k2, (unsigned)FS2, 1), tw_get(tw, (unsigned)k2, (unsigned)FS2, 2), tw_get(tw, (unsigned)k2, (unsigned)FS2, 3));
            }
#pragma unroll
            for (int j = 0; j < 16; ++j) Ls[F::phys(base + j * M)] = a[j];
        }
        fftp2_barrier<LB>();
        fftp2_rest<LOG2N, INV, 16 * M, TwPtr, LB>(Ls, tw, tid);
    } else if constexpr (M <= N / 4) { // one stage left
        constexpr int FS = N / (4 * M);
#pragma unroll 1
        for (int g = tid; g < E / 4; g += 256) {
            const int xf = g / (N / 4), gl = g % (N / 4);
            const int blk = gl / M, kk = gl % M;
            const int base = xf * N + blk * 4 * M + kk;
            float2 a0 = Ls[F::phys(base)], a1 = Ls[F::phys(base + M)], a2 = Ls[F::phys(base + 2 * M)], a3 = Ls[F::phys(base + 3 * M)];
            bfly4<INV>(a0, a1, a2, a3, tw_get(tw, (unsigned)kk, (unsigned)FS, 1), tw_get(tw, (unsigned)kk, (unsigned)FS, 2), tw_get(tw, (unsigned)kk, (unsigned)FS, 3));
            Ls[F::phys(base)] = a0; Ls[F::phys(base + M)] = a1; Ls[F::phys(base + 2 * M)] = a2; Ls[F::phys(base + 3 * M)] = a3;
        }
        fftp2_barrier<LB>();
    }
}

// every stage of the transforms of one workgroup image in LDS (leaf order in, natural order out); ends with a workgroup barrier
template <int LOG2N, bool INV, bool LB = false>
__device__ __forceinline__ void fftp2_lds_stages(float2 *Ls, const float2 *__restrict__ tw, const float2 *__restrict__ Tord, int tid)
{
    using F = FftP2<LOG2N>;
    constexpr int N = F::N, E = F::E;
    if constexpr (!F::ODD) {
        fftp2_rest<LOG2N, INV, 1, const float2 *, LB>(Ls, tw, tid); // powers of four: stages m = 1, 4, ... straight away
    } else if constexpr (N == 2) {
        for (int g = tid; g < E / 2; g += 256) {
            float2 a0 = Ls[F::phys(2 * g)], a1 = Ls[F::phys(2 * g + 1)];
            bfly2(a0, a1, tw[0]);
            Ls[F::phys(2 * g)] = a0; Ls[F::phys(2 * g + 1)] = a1;
        }
        fftp2_barrier<LB>();
    } else {
        // first pass: radix-2 (m = 1) then radix-4 (m = 2) on 8 consecutive positions
        constexpr int FS = N / 8;
        const float2 one = tw[0], w1 = tw[FS], w2 = tw[2 * FS], w3 = tw[3 * FS];
#pragma unroll 1
        for (int g = tid; g < E / 8; g += 256) {
            float2 a[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) a[j] = Ls[F::phys(8 * g + j)];
#pragma unroll
            for (int q = 0; q < 4; ++q) bfly2(a[2 * q], a[2 * q + 1], one);
            bfly4<INV>(a[0], a[2], a[4], a[6], one, one, one);
            bfly4<INV>(a[1], a[3], a[5], a[7], w1, w2, w3);
#pragma unroll
            for (int j = 0; j < 8; ++j) Ls[F::phys(8 * g + j)] = a[j];
        }
        fftp2_barrier<LB>();
        if constexpr (LOG2N == 9) fftp2_rest<LOG2N, INV, 8, TwProgram<512, 2>, LB>(Ls, TwProgram<512, 2>{Tord}, tid); // 512: the stage-ordered copy (+6 %; nothing below)
        else fftp2_rest<LOG2N, INV, 8, const float2 *, LB>(Ls, tw, tid);
    }
}

} // namespace redio
