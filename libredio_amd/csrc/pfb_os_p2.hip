// pfb_os_p2.hip -- the workgroup form of the oversampled channelizer (include/redio.h, redio_pfb_os_*, route 2; contract: DESIGN.md 5.6d)
// for 32, 128, 256, 512 or 1024 channels at a hop of half a row on gfx950 (pfb_bank.hip launches it).  Index maps, windows and stream
// geometry: pfb_os_p2_core.h.
//
// Algorithmic bytes: 8 B read from HBM + 16 B written per input sample (a row of M channels every M / 2 samples); 8 P + the transform's
// flop per sample.  Bound: HBM.
// pfb_os_p2_kernel is pfb_p2_kernel (pfb_p2.hip) behind the branch filters: the thread <-> branch map, the 4096-point LDS image of
// fft_p2.h, the twiddles in LDS, the two register sets swapping roles, the clamped loads on one path, the LDS-only barriers, the
// 16-byte non-temporal row stores.  In front of them the stream is read as overlapping half-rows s_q (M cf32 from (M / 2) q on): an
// output row brings ONE new half-row, so a thread issues one M-wide row load per output row as pfb_p2_kernel does, and keeps two
// register windows per channel, one for the even and one for the odd half-rows (pfb_os64_kernel at 64 channels).  Consecutive
// half-rows overlap by half: every sample is requested twice by the same workgroup, at most TR row loads apart, and the second
// request is served by the vector L1 or the L2.  The shift s_r (0 or M / 2) goes into the image position of the branch sum's store.
// A sibling and not a template parameter of pfb_p2_kernel: that kernel keeps its name and its code.
#include "redio_internal.h"
#include "../../include/redio.h"
#include "fft_p2.h"
#include "pfb_os_p2_core.h"

namespace redio {

bool pfb_p2_supported(int nchan, int taps_per_branch); // pfb_p2.hip

typedef float osp2_v2f __attribute__((ext_vector_type(2)));
typedef float osp2_v4f __attribute__((ext_vector_type(4)));

// PAIR: a thread owns two NEIGHBOURING channels (2 m, 2 m + 1) and loads them with one 16-byte access; the launcher chooses it only
// where x is 16-byte aligned (a half-row starts a whole number of 16-byte units behind x: M / 2 is even).  wide: `out` is 16-byte
// aligned (two neighbouring channels as one 16-byte store); otherwise two 8-byte stores.  fpar = first_row & 1.
template <int LOG2M, int P, bool FUSED, bool PAIR>
__global__ __launch_bounds__(256) void pfb_os_p2_kernel(const float2 *__restrict__ x, const float *__restrict__ h, const float2 *__restrict__ tw,
                                                        const float2 *__restrict__ Tord, float2 *__restrict__ out, long rows, long rps, int fpar, int wide)
{
    using F = FftP2<LOG2M>;
    constexpr int M = F::N;
    constexpr int NP = PAIR ? (M <= 512 ? 1 : M / 512) : (M <= 256 ? 1 : M / 256); // loads per thread and half-row
    constexpr int CPT = PAIR ? 2 * NP : NP, MT = M / CPT, G = 256 / MT, TR = 16 / CPT; // channels per thread, threads per row, streams, rows per iteration
    static_assert(F::E == 4096 && G * TR * M == 4096 && P >= 2 && P <= 16 && MT <= 256 && TR % 2 == 0, "shape");
    constexpr int HR = TR / 2; // rows of one parity per iteration
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2 *Ls = reinterpret_cast<float2 *>(smem);
    const int tid = threadIdx.x, m = tid % MT, g = tid / MT;
    auto chan = [&](int c) { return PAIR ? 2 * m + (c & 1) + 512 * (c >> 1) : m + 256 * c; }; // channel of slot c
    const long s0 = (long)blockIdx.x * G;                  // first stream of this workgroup: the one with the most rows
    const long t0 = pfbos_p2_stream_begin(s0 + g, rps);    // even: rps is a multiple of TR
    const int iters = (int)pfbos_p2_group_iters(blockIdx.x, rps, rows, M); // workgroup-uniform
    float gt[CPT][P];
#pragma unroll
    for (int c = 0; c < CPT; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p) gt[c][p] = h[M * p + chan(c)];
    float2 hist[CPT][2][P - 1], ra[CPT][TR], rb[CPT][TR];
    float2 *Ltw = Ls + F::LDS_ELEMS, *Ltord = Ltw + M; // pfb_p2_kernel: the transform's twiddles live in LDS
    for (int i = tid; i < M; i += 256) Ltw[i] = tw[i];
    if constexpr (LOG2M == 9)
        for (int i = tid; i < 510; i += 256) Ltord[i] = Tord[i];
    // half-rows past the last one the call may read are clamped by address (their rows are never stored); ONE path, never skipped
    // (pfb_p2_kernel: why)
    auto ld_half = [&](long q, float2 *dst /* [CPT], stride given by `step` */, int step) {
        const float2 *rowp = x + pfbos_p2_in_index(pfbos_p2_half(q, rows, P), 0, M);
#pragma unroll
        for (int u = 0; u < NP; ++u) {
            if constexpr (PAIR) {
                const osp2_v4f v = __builtin_nontemporal_load(reinterpret_cast<const osp2_v4f *>(rowp + 2 * m + 512 * u));
                dst[(2 * u) * step] = make_float2(v.x, v.y); dst[(2 * u + 1) * step] = make_float2(v.z, v.w);
            } else {
                const osp2_v2f v = __builtin_nontemporal_load(reinterpret_cast<const osp2_v2f *>(rowp + m + 256 * u));
                dst[u * step] = make_float2(v.x, v.y);
            }
        }
    };
#pragma unroll
    for (int p = 0; p < P - 1; ++p)
#pragma unroll
        for (int par = 0; par < 2; ++par) ld_half(pfbos_p2_hist_half(t0, par, p), &hist[0][par][p], 2 * (P - 1));
#pragma unroll
    for (int ti = 0; ti < TR; ++ti) ld_half(pfbos_p2_enter(t0 + ti, P), &ra[0][ti], TR);
    fftp2_barrier<true>(); // the twiddle copy is complete
    // one iteration: rows tb .. tb + TR - 1, whose entering half-rows are in `cur`; the next iteration's are requested into `nx`
    auto iteration = [&](int it, float2(&cur)[CPT][TR], float2(&nx)[CPT][TR]) {
        const long tb = t0 + (long)TR * it;
#pragma unroll
        for (int ti = 0; ti < TR; ++ti) ld_half(pfbos_p2_enter(tb + TR + ti, P), &nx[0][ti], TR);
#pragma unroll
        for (int c = 0; c < CPT; ++c) {
            // the branch sum's place in its row of the image, for even and for odd rows of the iteration: the shift is in the index
            const int lp[2] = {(TR * g) * M + pfbos_p2_image_pos<LOG2M>(chan(c), 0, fpar), (TR * g) * M + pfbos_p2_image_pos<LOG2M>(chan(c), 1, fpar)};
#pragma unroll
            for (int ti = 0; ti < TR; ++ti) { // output row tb + ti: half-rows tb + ti + 2 p, p = 0 .. P - 1 (its parity's window [hist | cur])
                const int par = ti & 1;
                float2 acc = make_float2(0.f, 0.f);
#pragma unroll
                for (int p = 0; p < P; ++p) {
                    const int k = pfbos_p2_win(ti, p);
                    acc = mac<FUSED>(k < P - 1 ? hist[c][par][k] : cur[c][pfbos_p2_cur_slot(par, k, P)], gt[c][p], acc);
                }
                Ls[F::phys(lp[par] + ti * M)] = acc;
            }
#pragma unroll
            for (int par = 0; par < 2; ++par) {
                float2 hn[P - 1]; // the last P - 1 half-rows of the parity's window
#pragma unroll
                for (int p = 0; p < P - 1; ++p) hn[p] = p + HR < P - 1 ? hist[c][par][p + HR] : cur[c][pfbos_p2_cur_slot(par, p + HR, P)];
#pragma unroll
                for (int p = 0; p < P - 1; ++p) hist[c][par][p] = hn[p];
            }
        }
        fftp2_barrier<true>();
        fftp2_lds_stages<LOG2M, false, true>(Ls, Ltw, Ltord, tid);
#pragma unroll 2
        for (int e = 2 * tid; e < 4096; e += 512) { // two neighbouring channels per thread: one 16-byte store where `out` allows it
            const int xf = e / M, n = e % M, gg = xf / TR, ti = xf % TR;
            const long row = pfbos_p2_stream_begin(s0 + gg, rps) + (long)TR * it + ti;
            if (row < pfbos_p2_stream_end(s0 + gg, rps, rows)) {
                const float2 v0 = Ls[F::phys(e)], v1 = Ls[F::phys(e + 1)];
                float2 *o = out + row * M + n;
                if (wide) {
                    __builtin_nontemporal_store(osp2_v4f{v0.x, v0.y, v1.x, v1.y}, reinterpret_cast<osp2_v4f *>(o));
                } else {
                    __builtin_nontemporal_store(osp2_v2f{v0.x, v0.y}, reinterpret_cast<osp2_v2f *>(o));
                    __builtin_nontemporal_store(osp2_v2f{v1.x, v1.y}, reinterpret_cast<osp2_v2f *>(o + 1));
                }
            }
        }
        fftp2_barrier<true>();
    };
    for (int it = 0; it < iters; it += 2) {
        iteration(it, ra, rb);
        if (it + 1 < iters) iteration(it + 1, rb, ra); // workgroup-uniform
    }
}

// pfb_p2_kernel's shapes at hop M / 2, but for 1024 channels x 16 taps: the two windows of a thread's four channels are 240 registers
// beside 64 taps and two sets of iteration rows, and that instantiation spills to scratch in both load forms (212-368 bytes a lane;
// with one set of iteration rows, and with the taps read per channel instead of resident, it still does: DESIGN.md 5.6d).  It is not
// built; the shape stays on route 0.
bool pfb_os_p2_supported(int nchan, int taps_per_branch, size_t hop)
{
    return pfb_p2_supported(nchan, taps_per_branch) && hop == (size_t)nchan / 2 && !(nchan == 1024 && taps_per_branch == 16);
}

template <int LOG2M, int P, bool PAIR>
static hipError_t launch_pfb_os_p2_t(const float2 *x, const float *h, const float2 *tw, const float2 *Tord, float2 *out, long rows, int fpar, bool fused,
                                     hipStream_t s)
{
    using F = FftP2<LOG2M>;
    constexpr int M = F::N;
    if (LOG2M == 9 && !Tord) return hipErrorInvalidValue;
    const size_t lds = (size_t)(F::LDS_ELEMS + (LOG2M == 9 ? 1022 : M)) * sizeof(float2); // pfb_p2_kernel's: the image and the twiddles
    const long rps = pfbos_p2_rows_per_stream(rows, num_cus(), M), grid = pfbos_p2_groups(rows, rps, M);
    if (grid > 0x7fffffffl) return hipErrorInvalidValue;
    const int wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (fused) hipLaunchKernelGGL((pfb_os_p2_kernel<LOG2M, P, true, PAIR>), dim3((unsigned)grid), dim3(256), lds, s, x, h, tw, Tord, out, rows, rps, fpar, wide);
    else hipLaunchKernelGGL((pfb_os_p2_kernel<LOG2M, P, false, PAIR>), dim3((unsigned)grid), dim3(256), lds, s, x, h, tw, Tord, out, rows, rps, fpar, wide);
    return hipGetLastError();
}

template <int L, int Q>
static hipError_t launch_pfb_os_p2_shape(bool pair, const float2 *x, const float *h, const float2 *tw, const float2 *Tord, float2 *out, long rows, int fpar,
                                         bool fused, hipStream_t s)
{
    if constexpr (L >= 9) {
        if (pair) return launch_pfb_os_p2_t<L, Q, true>(x, h, tw, Tord, out, rows, fpar, fused, s);
    }
    return launch_pfb_os_p2_t<L, Q, false>(x, h, tw, Tord, out, rows, fpar, fused, s);
}

// x: (M / 2) (rows - 1) + M P cf32 samples, 8-byte aligned; h: M P taps; tw: the M-entry forward table; Tord: the 512-point plan's
// stage-ordered copy (512 channels only); out: rows rows of M cf32, 8-byte aligned; first_row: F, of which only the parity matters at
// hop M / 2.  hipErrorNotSupported: no such shape
hipError_t launch_pfb_os_p2(const float2 *x, const float *h, const float2 *tw, const float2 *Tord, float2 *out, long rows, int nchan, int taps_per_branch,
                            uint64_t first_row, bool fused, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    if (!pfb_os_p2_supported(nchan, taps_per_branch, (size_t)nchan / 2)) return hipErrorNotSupported;
    const int fpar = (int)(first_row & 1);
    // the load form: two neighbouring channels per load where a thread owns several channels anyway (launch_pfb_p2: why) and x allows it
    const bool pair = nchan >= 512 && (reinterpret_cast<uintptr_t>(x) & 15) == 0;
#define REDIO_PFB_OS_P2(L, Q) \
    if (nchan == (1 << L) && taps_per_branch == Q) return launch_pfb_os_p2_shape<L, Q>(pair, x, h, tw, Tord, out, rows, fpar, fused, s);
    REDIO_PFB_OS_P2(5, 4) REDIO_PFB_OS_P2(5, 8) REDIO_PFB_OS_P2(5, 16) REDIO_PFB_OS_P2(7, 4) REDIO_PFB_OS_P2(7, 8) REDIO_PFB_OS_P2(7, 16)
    REDIO_PFB_OS_P2(8, 4) REDIO_PFB_OS_P2(8, 8) REDIO_PFB_OS_P2(8, 16) REDIO_PFB_OS_P2(9, 4) REDIO_PFB_OS_P2(9, 8) REDIO_PFB_OS_P2(9, 16)
    REDIO_PFB_OS_P2(10, 4) REDIO_PFB_OS_P2(10, 8)
#undef REDIO_PFB_OS_P2
    return hipErrorNotSupported;
}

} // namespace redio
