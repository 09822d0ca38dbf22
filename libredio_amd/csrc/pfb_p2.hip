// pfb_p2.hip -- the one-kernel polyphase channelizer for 32, 128, 256, 512 or 1024 channels (pfb_api.hip launches it): the branch
// filters write the LDS image of fft_p2.h, whose compile-time stages then transform it in place.
#include "redio_internal.h"
#include "../../include/redio.h"
#include "fft_p2.h"

namespace redio {

// ---- polyphase channelizer with M = 32, 128, 256, 512 or 1024 channels in ONE kernel (round 4): branch filters into the LDS image, then the
// M-point transform of fft_p2_kernel on the image, then the rows out -- 16 bytes per sample through HBM instead of the 32 of the two-pass
// form (pfb_api.hip: pfb_branch_kernel + the plan's transform).  v[t][m] = fold_p x[(t + p) M + m] * h[M p + m] (ascending p: dsputils.rs:31),
// kissfft's M-point forward transform across the branches of each row: the bits of oracle orc_pfb_channelizer.
// A workgroup iteration is 4096 points.  Up to 256 channels: 16 rows of each of its G = 256 / M row streams, thread (m, g) walks stream g;
// above: 4096 / M rows of ONE stream, a thread owns M / 256 channels.  A stream is a contiguous range of rows whose P - 1 rows of filter
// history are carried in registers, so an input row is loaded once (M * 8 contiguous bytes), and the next iteration's rows are requested
// before this one's arithmetic.
// PAIR: a thread owns two NEIGHBOURING channels (2 m, 2 m + 1) and loads them with one 16-byte access (M / 2 threads per row, so more
// row streams per workgroup and 8 rows per iteration); otherwise one channel per thread (or M / 256 channels, 256 apart), 8-byte loads.
#ifndef REDIO_EXP_PFB_NT
#define REDIO_EXP_PFB_NT 3 // bit 0: non-temporal row loads, bit 1: non-temporal row stores (pfb_kernels.hip: why)
#endif
typedef float p2_v2f __attribute__((ext_vector_type(2)));
typedef float p2_v4f __attribute__((ext_vector_type(4)));
template <int LOG2M, int P, bool FUSED, bool PAIR>
__global__ __launch_bounds__(256) void pfb_p2_kernel(const float2 *__restrict__ x, const float *__restrict__ h, const float2 *__restrict__ tw,
                                                     const float2 *__restrict__ Tord, float2 *__restrict__ out, long rows, long rps, int ngroups)
{
    using F = FftP2<LOG2M>;
    constexpr int M = F::N;
    constexpr int NP = PAIR ? (M <= 512 ? 1 : M / 512) : (M <= 256 ? 1 : M / 256); // loads per thread and row
    constexpr int CPT = PAIR ? 2 * NP : NP, MT = M / CPT, G = 256 / MT, TR = 16 / CPT; // channels per thread, threads per row, streams, rows per iteration
    static_assert(F::E == 4096 && G * TR * M == 4096 && P >= 2 && P <= 16 && MT <= 256, "shape");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *Ls = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x, m = tid % MT, g = tid / MT;
    auto chan = [&](int c) { return PAIR ? 2 * m + (c & 1) + 512 * (c >> 1) : m + 256 * c; }; // channel of slot c
    const long s0 = (long)blockIdx.x * G;                 // first stream of this workgroup: the one with the most rows
    const long t0 = (s0 + g) * rps, last_in_row = rows + P - 2;
    const long rows0 = (s0 * rps + rps < rows ? rps : rows - s0 * rps);
    const int iters = (int)((rows0 + TR - 1) / TR);       // workgroup-uniform
    float gt[CPT][P];
#pragma unroll
    for (int c = 0; c < CPT; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p) gt[c][p] = h[M * p + chan(c)];
    float2 hist[CPT][P - 1], ra[CPT][TR], rb[CPT][TR];
    // The transform's twiddles live in LDS for the life of the workgroup (round 5): read from global memory inside the stages they are vector
    // loads whose wait (vmcnt: loads return in order) also waits for the NEXT iteration's rows requested at the top of this one -- and every
    // barrier below is an LDS-only barrier for the same reason (__syncthreads() waits for all requests in flight).  M <= 1024 entries.
    float2 *Ltw = Ls + F::LDS_ELEMS, *Ltord = Ltw + M; // the M-entry table; for 512 channels also the stage-ordered copy (510 entries) behind it
    for (int i = tid; i < M; i += 256) Ltw[i] = tw[i];
    if constexpr (LOG2M == 9)
        for (int i = tid; i < 510; i += 256) Ltord[i] = Tord[i];
    // rows past the stream's end are clamped (their outputs are never stored); ONE path, never skipped: the compiler can then count the
    // requests in flight at every use instead of waiting for all of them
    auto ld_row = [&](long r, float2 *dst /* [CPT], stride given by `step` */, int step) {
        const float2 *rowp = x + (long)M * (r < last_in_row ? r : last_in_row);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if (PAIR) {
#if REDIO_EXP_PFB_NT & 1
                const p2_v4f v = __builtin_nontemporal_load(reinterpret_cast<const p2_v4f *>(rowp + 2 * m + 512 * q));
#else
                const float4 v = *reinterpret_cast<const float4 *>(rowp + 2 * m + 512 * q);
#endif
                dst[(2 * q) * step] = make_float2(v.x, v.y); dst[(2 * q + 1) * step] = make_float2(v.z, v.w);
            } else {
#if REDIO_EXP_PFB_NT & 1
                const p2_v2f v = __builtin_nontemporal_load(reinterpret_cast<const p2_v2f *>(rowp + m + 256 * q));
                dst[q * step] = make_float2(v.x, v.y);
#else
                dst[q * step] = rowp[m + 256 * q];
#endif
            }
        }
    };
#pragma unroll
    for (int p = 0; p < P - 1; ++p) ld_row(t0 + p, &hist[0][p], P - 1);
#pragma unroll
    for (int ti = 0; ti < TR; ++ti) ld_row(t0 + P - 1 + ti, &ra[0][ti], TR);
    const int cpg = M / ngroups;
    fftp2_barrier<true>(); // the twiddle copy is complete
    // one iteration: rows tb .. tb + TR - 1 from `cur`, the next iteration's rows requested into `nx` (the loop below is unrolled by two with
    // the two register sets swapping roles: a copy nx -> cur of a loop-carried array lands behind the iteration's stores and waits for them)
    auto iteration = [&](int it, float2(&cur)[CPT][TR], float2(&nx)[CPT][TR]) {
        const long tb = t0 + (long)TR * it;
#pragma unroll
        for (int ti = 0; ti < TR; ++ti) ld_row(tb + TR + P - 1 + ti, &nx[0][ti], TR);
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            const int lp = (TR * g) * M + F::leaf_pos(chan(c));
#pragma unroll
            for (int ti = 0; ti < TR; ++ti) { // output row tb + ti: input rows tb + ti + p, p = 0 .. P - 1 (the window is [hist | cur])
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int p = 0; p < P; ++p) acc = mac<FUSED>(ti + p < P - 1 ? hist[c][ti + p] : cur[c][ti + p - (P - 1)], gt[c][p], acc);
                Ls[F::phys(lp + ti * M)] = acc;
            }
            float2 hn[P - 1]; // the last P - 1 rows of [hist | cur]
#pragma unroll
            for (int p = 0; p < P - 1; ++p) hn[p] = p + TR < P - 1 ? hist[c][p + TR] : cur[c][p + TR - (P - 1)];
#pragma unroll
            for (int p = 0; p < P - 1; ++p) hist[c][p] = hn[p];
        }
        fftp2_barrier<true>();
        fftp2_lds_stages<LOG2M, false, true>(Ls, Ltw, Ltord, tid);
#pragma unroll 2
        for (int e = 2 * tid; e < 4096; e += 512) { // two neighbouring channels per thread: one 16-byte store
            const int xf = e / M, n = e % M, gg = xf / TR, ti = xf % TR;
            const long sbase = (s0 + gg) * rps, row = sbase + (long)TR * it + ti, rend = sbase + rps < rows ? sbase + rps : rows;
            if (row < rend) {
                const float2 v0 = Ls[F::phys(e)], v1 = Ls[F::phys(e + 1)];
                float2 *o16 = ngroups == 1 ? out + row * M + n : out + (long)(n / cpg) * rows * cpg + row * cpg + (n % cpg);
                if (ngroups == 1 || cpg >= 2) {
#if REDIO_EXP_PFB_NT & 2
                    __builtin_nontemporal_store(p2_v4f{v0.x, v0.y, v1.x, v1.y}, reinterpret_cast<p2_v4f *>(o16));
#else
                    *reinterpret_cast<float4 *>(o16) = make_float4(v0.x, v0.y, v1.x, v1.y);
#endif
                }
                else { out[(long)n * rows + row] = v0; out[(long)(n + 1) * rows + row] = v1; }
            }
        }
        fftp2_barrier<true>();
    };
    for (int it = 0; it < iters; it += 2) {
        iteration(it, ra, rb);
        if (it + 1 < iters) iteration(it + 1, rb, ra); // workgroup-uniform
    }
}

bool pfb_p2_supported(int nchan, int taps_per_branch)
{
    return (nchan == 32 || nchan == 128 || nchan == 256 || nchan == 512 || nchan == 1024) && (taps_per_branch == 4 || taps_per_branch == 8 || taps_per_branch == 16);
}
template <int LOG2M, int P, bool PAIR>
static hipError_t launch_pfb_p2_t(const float2 *x, const float *h, const float2 *tw, const float2 *Tord, float2 *out, long rows, int ngroups, bool fused,
                                  hipStream_t s)
{
    using F = FftP2<LOG2M>;
    constexpr int M = F::N, NP = PAIR ? (M <= 512 ? 1 : M / 512) : (M <= 256 ? 1 : M / 256), CPT = PAIR ? 2 * NP : NP, G = 256 / (M / CPT), TR = 16 / CPT;
    if (LOG2M == 9 && !Tord) return hipErrorInvalidValue;
    // the image + the twiddles the shape needs (M entries; 512 channels: + the 510-entry stage-ordered copy).  Round 5 reserved 1024 entries
    // for every shape: 45.1 KB, three workgroups per CU where four were launched (advisor, round 5); now 37.2-39 KB up to 256 channels
    const size_t lds = (size_t)(F::LDS_ELEMS + (LOG2M == 9 ? 1022 : M)) * sizeof(float2);
    // contiguous row ranges per stream, a multiple of the iteration's rows; about four workgroups per CU -- also for 512 / 1024 channels,
    // where three are resident: sized for three the launch is 16 % SLOWER (0.866 -> 1.027 ms, profiles/r06_c4gen_ab.txt: the fourth
    // quarter of the streams is what evens out the tail); at least 64 rows (the P - 1 row prologue)
    long streams = 4L * num_cus() * G;
    long rps = (rows + streams - 1) / streams;
    rps = ((rps + TR - 1) / TR) * TR;
    if (rps < 64) rps = 64;
    const long nstreams = (rows + rps - 1) / rps;
    const unsigned grid = (unsigned)((nstreams + G - 1) / G);
    if (fused) hipLaunchKernelGGL((pfb_p2_kernel<LOG2M, P, true, PAIR>), dim3(grid), dim3(256), lds, s, x, h, tw, Tord, out, rows, rps, ngroups);
    else hipLaunchKernelGGL((pfb_p2_kernel<LOG2M, P, false, PAIR>), dim3(grid), dim3(256), lds, s, x, h, tw, Tord, out, rows, rps, ngroups);
    return hipGetLastError();
}
// out: [row][M] (ngroups == 1) or [group][row][M / ngroups]; tw: the M-entry forward table; Tord: the 512-point plan's stage-ordered copy (512 channels only)
hipError_t launch_pfb_p2(const float2 *x, const float *h, const float2 *tw, const float2 *Tord, float2 *out, long rows, int nchan, int taps_per_branch,
                         int ngroups, bool fused, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    if (!pfb_p2_supported(nchan, taps_per_branch) || ngroups < 1 || nchan % ngroups) return hipErrorNotSupported;
    if ((reinterpret_cast<uintptr_t>(out) & 15) != 0) return hipErrorNotSupported; // 16-byte stores
    // 16-byte row loads (two neighbouring channels per thread, 16-byte aligned input) where a thread owns several channels anyway: 512 channels
    // 0.993 -> 0.972 ms, 1024 channels 1.031 -> 0.957 ms per 2^28 samples; up to 256 channels the second channel's window costs more registers
    // than the wider load saves (256 channels, 16 taps: 0.96 -> 1.57 ms), so those keep one channel per thread (profiles/r04_channelizer_pair_loads_ab.txt).
    // Measurement builds: REDIO_PFB_NO_PAIR forces the 8-byte form, REDIO_PFB_PAIR the 16-byte form
    const bool pair = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && (nchan >= 512 || measure_env("REDIO_PFB_PAIR")) && !measure_env("REDIO_PFB_NO_PAIR");
#define REDIO_PFB_P2(L, Q)                                                                                                    \
    if (nchan == (1 << L) && taps_per_branch == Q)                                                                            \
        return pair ? launch_pfb_p2_t<L, Q, true>(x, h, tw, Tord, out, rows, ngroups, fused, s) : launch_pfb_p2_t<L, Q, false>(x, h, tw, Tord, out, rows, ngroups, fused, s);
    REDIO_PFB_P2(5, 4) REDIO_PFB_P2(5, 8) REDIO_PFB_P2(5, 16) REDIO_PFB_P2(7, 4) REDIO_PFB_P2(7, 8) REDIO_PFB_P2(7, 16) REDIO_PFB_P2(8, 4) REDIO_PFB_P2(8, 8) REDIO_PFB_P2(8, 16)
    REDIO_PFB_P2(9, 4) REDIO_PFB_P2(9, 8) REDIO_PFB_P2(9, 16) REDIO_PFB_P2(10, 4) REDIO_PFB_P2(10, 8) REDIO_PFB_P2(10, 16)
#undef REDIO_PFB_P2
    return hipErrorNotSupported;
}

} // namespace redio
