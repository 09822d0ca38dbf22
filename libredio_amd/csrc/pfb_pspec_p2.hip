// pfb_pspec_p2.hip -- the workgroup form of the polyphase spectrometer (redio_pfb_pspec_*, route 2; contract: DESIGN.md 5.6b) for 32,
// 128, 256, 512 or 1024 channels on gfx950.  Thread programs and stream geometry: pfb_pspec_p2_core.h.
//
// Algorithmic bytes: 8 B (cf32) or 2 B (u8 I/Q) read per input sample + 4 / K written.
// pfbspec_p2_kernel is pfb_p2_kernel (pfb_p2.hip) up to the end of the transform: the twiddles in LDS, the register window
// [hist | cur], the two register sets swapping roles, the clamped loads on one path, the LDS-only barriers.  Behind the transform the
// image holds bin n of local row xf at Ls[F::phys(xf * M + n)]; instead of storing it, the thread that filtered a channel reads that
// channel's bin of each of its stream's rows, squares it and steps the fold of pspec_core.h, accumulators in registers.
// A sibling and not a template parameter of pfb_p2_kernel: that kernel keeps its name and its code.
#include "redio_internal.h"
#include "../../include/redio.h"
#include "fft_p2.h"
#include "pfb_pspec_p2_core.h"
#include <type_traits>

namespace redio {

typedef float psp2_v2f __attribute__((ext_vector_type(2)));
typedef float psp2_v4f __attribute__((ext_vector_type(4)));

// what one row load of a thread brings: one sample, or with PAIR two neighbouring channels' (16 bytes of cf32, 4 bytes of u8 I/Q)
template <bool PAIR, bool IN_U8>
struct PfbSpecP2Raw {
    using type = std::conditional_t<IN_U8, std::conditional_t<PAIR, unsigned, unsigned short>, std::conditional_t<PAIR, psp2_v4f, psp2_v2f>>;
};

// A stream owns units [u0, u1) of the launch (pfbspec_p2_stream), which are the consecutive channelizer rows [t0, t1); `rows` = every
// channelizer row the launch sums (the input holds rows + P - 1 rows of samples).  dst: M f32 per unit (the output rows, or the
// segment partials).  IN_U8: x is the receiver's interleaved u8 I/Q bytes, one 16-bit word per sample, converted by i2f() where the
// branch filters read it.  PAIR: two neighbouring channels per load; the launcher chooses it only where x is aligned for it.
template <int LOG2M, int P, bool FUSED, bool PAIR, bool IN_U8>
__global__ __launch_bounds__(256) void pfbspec_p2_kernel(const void *__restrict__ xv, const float *__restrict__ h, const float2 *__restrict__ tw,
                                                         const float2 *__restrict__ Tord, float *__restrict__ dst, long rows, long nunits,
                                                         long ups, long K, int split)
{
    using F = FftP2<LOG2M>;
    constexpr int M = F::N;
    constexpr int NP = PAIR ? (M <= 512 ? 1 : M / 512) : (M <= 256 ? 1 : M / 256); // loads per thread and row
    constexpr int CPT = PAIR ? 2 * NP : NP, MT = M / CPT, G = 256 / MT, TR = 16 / CPT; // channels per thread, threads per row, streams, rows per iteration
    static_assert(F::E == 4096 && G * TR * M == 4096 && P >= 2 && P <= 16 && MT <= 256 && G <= 8, "shape");
    using raw_t = typename PfbSpecP2Raw<PAIR, IN_U8>::type;
    using elem_t = std::conditional_t<IN_U8, unsigned short, float2>; // one sample as it lies in memory
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *Ls = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x, m = tid % MT;
    // the stream, and with it the fold's counters, is wave-uniform from 64 threads per row up; at 32 channels a wave holds two streams
    const int g = MT >= 64 ? __builtin_amdgcn_readfirstlane(tid / MT) : tid / MT;
    auto chan = [&](int c) { return PAIR ? 2 * m + (c & 1) + 512 * (c >> 1) : m + 256 * c; }; // channel of slot c
    const PfbSpecP2Stream st = pfbspec_p2_stream((long)blockIdx.x * G + g, ups, nunits, rows, K, split != 0);
    const long t0 = st.t0, t1 = st.t1, last_in_row = rows + P - 2; // the last row of samples the launch may read
    PfbSpecFold fold;
    {
        long tf;
        pfbspec_fold_begin(fold, st.u0, K, split != 0, tf);
    }
    float gt[CPT][P];
#pragma unroll
    for (int c = 0; c < CPT; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p) gt[c][p] = h[M * p + chan(c)];
    float2 hist[CPT][P - 1];
    raw_t ra[NP][TR], rb[NP][TR];
    float2 *Ltw = Ls + F::LDS_ELEMS, *Ltord = Ltw + M; // pfb_p2_kernel: the transform's twiddles live in LDS
    for (int i = tid; i < M; i += 256) Ltw[i] = tw[i];
    if constexpr (LOG2M == 9)
        for (int i = tid; i < 510; i += 256) Ltord[i] = Tord[i];
    // The iteration count is the workgroup's: the maximum over its streams (with `split` a row's last segment is short, so the streams
    // of a workgroup can hold different numbers of rows).  Exchanged through the eight words behind the image's last element
    // (F::phys(4095) = 4606 < LDS_ELEMS - 4), which nothing else touches.
    int *Lit = reinterpret_cast<int *>(Ls + F::LDS_ELEMS - 4);
    if (m == 0) Lit[g] = (int)pfbspec_p2_stream_iters(st, TR);
    const elem_t *x = reinterpret_cast<const elem_t *>(xv);
    // rows past the stream's end are clamped (they are never summed); ONE path, never skipped (pfb_p2_kernel: why)
    auto ld_row = [&](long r, raw_t *dstr /* [NP], stride given by `step` */, int step) {
        const elem_t *rowp = x + (long)M * (r < last_in_row ? r : last_in_row);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            if constexpr (PAIR) dstr[q * step] = __builtin_nontemporal_load(reinterpret_cast<const raw_t *>(rowp + 2 * m + 512 * q));
            else dstr[q * step] = __builtin_nontemporal_load(reinterpret_cast<const raw_t *>(rowp + m + 256 * q));
        }
    };
    // sample of channel slot c out of the thread's loads of one row
    auto sample = [](const raw_t &w, int c) -> float2 {
        if constexpr (IN_U8) {
            const unsigned v = PAIR ? ((unsigned)w >> (16 * (c & 1))) & 0xffffu : (unsigned)w;
            return make_float2(i2f(v & 255u), i2f(v >> 8));
        } else if constexpr (PAIR) {
            return (c & 1) ? make_float2(w.z, w.w) : make_float2(w.x, w.y);
        } else {
            return make_float2(w.x, w.y);
        }
    };
    constexpr int LQ = PAIR ? 2 : 1; // channel slots per load
    {
        raw_t hr[NP][P - 1];
#pragma unroll
        for (int p = 0; p < P - 1; ++p) ld_row(t0 + p, &hr[0][p], P - 1);
#pragma unroll
        for (int ti = 0; ti < TR; ++ti) ld_row(t0 + P - 1 + ti, &ra[0][ti], TR);
#pragma unroll
        for (int c = 0; c < CPT; ++c)
#pragma unroll
            for (int p = 0; p < P - 1; ++p) hist[c][p] = sample(hr[c / LQ][p], c);
    }
    float seg[CPT], row[CPT]; // this thread's channels: the segment and the unit being summed
#pragma unroll
    for (int c = 0; c < CPT; ++c) seg[c] = row[c] = 0.f;
    [[maybe_unused]] const bool dst8 =(reinterpret_cast<uintptr_t>(dst) & 7) == 0;
    fftp2_barrier<true>(); // the twiddle copy and the iteration counts are complete
    int iters = 0;
#pragma unroll
    for (int gg = 0; gg < G; ++gg) iters = Lit[gg] > iters ? Lit[gg] : iters;
    iters = __builtin_amdgcn_readfirstlane(iters); // workgroup-uniform
    // one iteration: rows tb .. tb + TR - 1 from `cur`, the next iteration's rows requested into `nx`
    auto iteration = [&](int it, raw_t(&cur)[NP][TR], raw_t(&nx)[NP][TR]) {
        const long tb = t0 + (long)TR * it;
#pragma unroll
        for (int ti = 0; ti < TR; ++ti) ld_row(tb + TR + P - 1 + ti, &nx[0][ti], TR);
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            const int lp = (TR * g) * M + F::leaf_pos(chan(c));
            float2 cv[TR];
#pragma unroll
            for (int ti = 0; ti < TR; ++ti) cv[ti] = sample(cur[c / LQ][ti], c);
#pragma unroll
            for (int ti = 0; ti < TR; ++ti) { // output row tb + ti: input rows tb + ti + p, p = 0 .. P - 1 (the window is [hist | cur])
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int p = 0; p < P; ++p) acc = mac<FUSED>(ti + p < P - 1 ? hist[c][ti + p] : cv[ti + p - (P - 1)], gt[c][p], acc);
                Ls[F::phys(lp + ti * M)] = acc;
            }
            float2 hn[P - 1]; // the last P - 1 rows of [hist | cur]
#pragma unroll
            for (int p = 0; p < P - 1; ++p) hn[p] = p + TR < P - 1 ? hist[c][p + TR] : cv[p + TR - (P - 1)];
#pragma unroll
            for (int p = 0; p < P - 1; ++p) hist[c][p] = hn[p];
        }
        fftp2_barrier<true>();
        fftp2_lds_stages<LOG2M, false, true>(Ls, Ltw, Ltord, tid);
        // the thread's own channels of its stream's TR rows, squared; the image is free for the next iteration behind these reads
        float pw[TR][CPT];
#pragma unroll
        for (int ti = 0; ti < TR; ++ti)
#pragma unroll
            for (int c = 0; c < CPT; ++c) pw[ti][c] = pspec_power(Ls[F::phys((TR * g + ti) * M + chan(c))]);
        fftp2_barrier<true>();
#pragma unroll
        for (int ti = 0; ti < TR; ++ti) {
            if (tb + ti < t1) { // stream-uniform
                const PspecStep ps = pspec_step(fold.i, fold.cnt);
#pragma unroll
                for (int c = 0; c < CPT; ++c) pfbspec_p2_fold_accum(ps, pw[ti][c], seg[c], row[c]);
                if (pfbspec_p2_fold_ends(fold)) { // the unit's last row: consecutive threads, consecutive words
                    float *d = dst + fold.u * M;
                    bool wide = false;
                    if constexpr (PAIR) { // the thread's two neighbouring channels as one 8-byte store where dst allows it
                        wide = dst8;
                        if (wide) {
#pragma unroll
                            for (int q = 0; q < NP; ++q) *reinterpret_cast<float2 *>(d + chan(2 * q)) = make_float2(row[2 * q], row[2 * q + 1]);
                        }
                    }
                    if (!wide) {
#pragma unroll
                        for (int c = 0; c < CPT; ++c) d[chan(c)] = row[c];
                    }
                }
                pfbspec_p2_fold_next(fold, K, split != 0);
            }
        }
    };
    for (int it = 0; it < iters; it += 2) {
        iteration(it, ra, rb);
        if (it + 1 < iters) iteration(it + 1, rb, ra); // workgroup-uniform
    }
}

template <int LOG2M, int P, bool PAIR, bool IN_U8>
static hipError_t launch_pfbspec_p2_t(const void *x, const float *h, const float2 *tw, const float2 *Tord, float *dst, long nunits, long K, bool split,
                                      bool fused, hipStream_t s)
{
    using F = FftP2<LOG2M>;
    constexpr int M = F::N;
    if (LOG2M == 9 && !Tord) return hipErrorInvalidValue;
    const size_t lds = (size_t)(F::LDS_ELEMS + (LOG2M == 9 ? 1022 : M)) * sizeof(float2); // pfb_p2_kernel's: the image and the twiddles
    const long rows = (split ? nunits / pspec_nseg(K) : nunits) * K; // a launch holds whole output rows
    const long ups = pfbspec_p2_units_per_stream(nunits, K, split, num_cus(), M);
    const long nstreams = (nunits + ups - 1) / ups;
    const int G = pfbspec_p2_streams_per_group(M);
    const long grid = (nstreams + G - 1) / G;
    if (grid > 0x7fffffffl) return hipErrorInvalidValue;
    if (fused)
        hipLaunchKernelGGL((pfbspec_p2_kernel<LOG2M, P, true, PAIR, IN_U8>), dim3((unsigned)grid), dim3(256), lds, s, x, h, tw, Tord, dst, rows, nunits, ups, K,
                           split ? 1 : 0);
    else
        hipLaunchKernelGGL((pfbspec_p2_kernel<LOG2M, P, false, PAIR, IN_U8>), dim3((unsigned)grid), dim3(256), lds, s, x, h, tw, Tord, dst, rows, nunits, ups, K,
                           split ? 1 : 0);
    return hipGetLastError();
}

// the load form: two neighbouring channels per load where a thread owns several channels anyway (launch_pfb_p2: why) and `pair`
// says that the base allows it
template <int L, int Q>
static hipError_t launch_pfbspec_p2_shape(const void *x, bool in_u8, bool pair, const float *h, const float2 *tw, const float2 *Tord, float *dst, long nunits,
                                          long K, bool split, bool fused, hipStream_t s)
{
    if constexpr (L >= 9) {
        if (pair)
            return in_u8 ? launch_pfbspec_p2_t<L, Q, true, true>(x, h, tw, Tord, dst, nunits, K, split, fused, s)
                         : launch_pfbspec_p2_t<L, Q, true, false>(x, h, tw, Tord, dst, nunits, K, split, fused, s);
    }
    return in_u8 ? launch_pfbspec_p2_t<L, Q, false, true>(x, h, tw, Tord, dst, nunits, K, split, fused, s)
                 : launch_pfbspec_p2_t<L, Q, false, false>(x, h, tw, Tord, dst, nunits, K, split, fused, s);
}

// x: cf32 samples (8-byte aligned) or, with in_u8, u8 I/Q byte pairs (2-byte aligned); nunits: output rows, or with `split` their
// segments (a whole number of rows' worth); dst: nchan f32 per unit; tw: the nchan-entry forward table; Tord: the 512-point plan's
// stage-ordered copy (512 channels only).  hipErrorNotSupported: no such shape
hipError_t launch_pfbspec_p2(const void *x, bool in_u8, const float *h, const float2 *tw, const float2 *Tord, float *dst, long nunits, long K, int nchan,
                             int taps_per_branch, bool split, bool fused, hipStream_t s)
{
    if (nunits <= 0) return hipSuccess;
    if (!pfb_p2_supported(nchan, taps_per_branch)) return hipErrorNotSupported;
    const bool pair = nchan >= 512 && (reinterpret_cast<uintptr_t>(x) & (in_u8 ? 3 : 15)) == 0; // 16 bytes of cf32, 4 bytes of u8 I/Q
#define REDIO_PFBSPEC_P2(L, Q) \
    if (nchan == (1 << L) && taps_per_branch == Q) return launch_pfbspec_p2_shape<L, Q>(x, in_u8, pair, h, tw, Tord, dst, nunits, K, split, fused, s);
    REDIO_PFBSPEC_P2(5, 4) REDIO_PFBSPEC_P2(5, 8) REDIO_PFBSPEC_P2(5, 16) REDIO_PFBSPEC_P2(7, 4) REDIO_PFBSPEC_P2(7, 8) REDIO_PFBSPEC_P2(7, 16)
    REDIO_PFBSPEC_P2(8, 4) REDIO_PFBSPEC_P2(8, 8) REDIO_PFBSPEC_P2(8, 16) REDIO_PFBSPEC_P2(9, 4) REDIO_PFBSPEC_P2(9, 8) REDIO_PFBSPEC_P2(9, 16)
    REDIO_PFBSPEC_P2(10, 4) REDIO_PFBSPEC_P2(10, 8) REDIO_PFBSPEC_P2(10, 16)
#undef REDIO_PFBSPEC_P2
    return hipErrorNotSupported;
}

} // namespace redio
