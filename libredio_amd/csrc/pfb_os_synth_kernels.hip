// pfb_os_synth_kernels.hip -- 64-channel oversampled synthesis bank at hop 32 (include/redio_pfb_os_synth.h, redio_pfb_os_synth_*, route 1) on gfx950.
// Index maps, launch geometry and the arithmetic contract: pfb_os_synth_core.h.
//
// Algorithmic bytes: 8 B read + 4 B written per channel value (a row of 64 values makes 32 samples); 4 P + 30 flop per value (+ the
// halo's transforms: two tiles per wave at P = 16).  Bound: HBM.  pfb_synth64_kernel (pfb_synth_kernels.hip) up to exchange 3 -- each
// wavefront owns a contiguous run of output hops, loads every input row once as 512 contiguous bytes per wave instruction and takes
// tiles of 16 rows through the INV = true lane programs -- then the hop-32 overlap-add: rows in pairs, the half of the wave whose hop
// completes first reads the tile one row behind the other half, both halves fold the same 2 P window registers with the same 2 P taps,
// and a pair's 64 results are one 512-byte store.  No scratch, no workgroup barrier: a wave's LDS tile is its own.
#include "fft_wave.h"
#include "pfb_wave.h"
#include "pfb_os_synth_core.h"
#include "redio_internal.h"
#include <type_traits>

namespace redio {

template <int P, bool FUSED>
__global__ __launch_bounds__(256) void pfb_os_synth64_kernel(const float2 *__restrict__ x, const float *__restrict__ h, const float2 *__restrict__ tw,
                                                             float2 *__restrict__ out, long hops, long hops_per_wave, int fpar)
{
    constexpr int L = 2 * P;
    static_assert((2 * PFB_TILE) % L == 0, "two tiles move the window by 32 slots: it rotates in place only if 2 P divides 32");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *lds = reinterpret_cast<float2 *>(smem) + wave * PFB_LDS;
    const long t0 = ((long)blockIdx.x * 4 + wave) * hops_per_wave; // output hops [t0, t1); t0 is even
    if (t0 >= hops) return; // wave-uniform; no workgroup barrier in this kernel
    const long t1 = (t0 + hops_per_wave < hops) ? t0 + hops_per_wave : hops;
    const long r_end = t1 + L - 1; // input rows [t0, r_end)
    const int early = pfboss_early(lane, fpar);

    float g[L];
#pragma unroll
    for (int k = 0; k < L; ++k) g[k] = h[pfboss_tap64(lane, k)];
    // ONE straight-line path, as pfb_synth64_kernel's load_rows: a row past the end of the call is clamped with scalar arithmetic
    float2 rows[PFB_TILE];
    auto load_rows = [&](float2(&dst)[PFB_TILE], long first) {
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) dst[ti] = x[PFB_M * pfboss_in_row(first + ti, hops, P) + (unsigned)lane];
    };
    // the inverse transform's twiddles, once per wavefront (pfb_core.h: why not inside the tile loop): 20 scalar and 24 vector registers
    PFB_WAVE_TWIDDLES(tw, lane);
    load_rows(rows, t0);
    // the window and the row carried from the tile before: the halo's outputs are never stored, any finite start will do
    float2 win[L], carry = make_float2(0.f, 0.f);
#pragma unroll
    for (int k = 0; k < L; ++k) win[k] = make_float2(0.f, 0.f);
    // where a lane's rows and its sample are: the early half reads exchange 3's tile one row behind the other half and writes the first
    // 32 samples of a pair's 64 (pfb_os_synth_core.h)
    const int x3 = pfboss_x3_base(lane, early);
    const unsigned opos = (unsigned)pfboss_out_pos(lane, early);
    // One tile: input rows rb .. rb + 15 from `rows`; the next tile's rows are requested into the same registers as soon as exchange 1
    // has taken these (one register set, not pfb_synth64_kernel's two: the window and the taps are twice as long here, and the second
    // set would put P = 16 at one wavefront per SIMD), and arrive under the transform and the overlap-add.  The tile loop is unrolled by
    // two: `par` is the tile's parity inside the run, which makes every window slot a compile-time constant at all three P.
    auto tile = [&](long rb, auto par) {
        constexpr int PAR = decltype(par)::value;
        // exchange 1: lane = channel -> the transform's layout
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) lds[pfb_x1_store(ti, lane)] = rows[ti];
        wave_lds_fence();
        load_rows(rows, rb + PFB_TILE);
        float2 v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = lds[pfb_x1_load(lane, e)];
        wave_lds_fence();
        pfb_fft64_passAB_pre<true>(v, twone, twa1, twa2, twa3);
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2)
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) lds[pfb_x2_store(lane, k1, k2)] = v[k1 + 4 * k2];
        wave_lds_fence();
#pragma unroll
        for (int f = 0; f < 16; ++f) v[f] = lds[pfb_x2_load(lane, f)];
        wave_lds_fence();
        pfb_fft64_passC_pre<true>(v, twc1, twc2, twc3);
        // exchange 3: lane (tt, k1) holding w[k2 + 4 k1 + 16 k0] -> lane = column
#pragma unroll
        for (int k0 = 0; k0 < 4; ++k0)
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) lds[pfbs_x3_store(lane, k0, k2)] = v[k0 + 4 * k2];
        wave_lds_fence();
        // overlap-add: the pair of rows (rb + 2 u, rb + 2 u + 1) completes one hop in every lane; strict fold over k (dsputils.rs:31)
#pragma unroll
        for (int u = 0; u < PFB_TILE / 2; ++u) {
            const int ti = 2 * u, s = pfboss_slot_new(PAR, u, P);
            if (u == 0) {
                const float2 first = lds[pfbs_x3_load(0, lane)];
                win[s] = make_float2(early ? carry.x : first.x, early ? carry.y : first.y);
            } else {
                win[s] = lds[pfboss_x3_load(x3, ti)];
            }
            win[s + 1] = lds[pfboss_x3_load(x3, ti + 1)];
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int k = 0; k < L; ++k) acc = mac<FUSED>(win[pfboss_slot(PAR, u, k, P)], g[k], acc);
            const long q0 = pfboss_hop(rb + ti, P); // the early half's hop; the other half's is q0 + 1: 64 consecutive samples from 32 q0 on
            const bool st_early = q0 >= t0 && q0 < t1, st_late = q0 + 1 >= t0 && q0 + 1 < t1; // wave-uniform
            if (early ? st_early : st_late) out[PFBOS_H * q0 + opos] = acc; // 512 bytes per instruction inside a run, 256 at its two ends
        }
        carry = lds[pfbs_x3_load(PFB_TILE - 1, lane)];
        wave_lds_fence(); // the next tile's exchange 1 overwrites what the overlap-add has just read
    };
    for (long rb = t0; rb < r_end; rb += 2 * PFB_TILE) {
        tile(rb, std::integral_constant<int, 0>{});
        if (rb + PFB_TILE < r_end) tile(rb + PFB_TILE, std::integral_constant<int, 1>{});
    }
}

// Route 0's second pass: one thread per output sample n = q H + j over the transformed rows w [rows][M] of a pass, the contract's fold
// with every index in 64-bit.  f0 = (F + the pass's first row) mod M.
template <bool FUSED>
__global__ __launch_bounds__(256) void pfb_os_synth_ola_kernel(const float2 *__restrict__ w, const float *__restrict__ h, float2 *__restrict__ out, long nout,
                                                               long M, long P, long H, long L, long f0)
{
    const long n = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nout) return;
    const long q = n / H, j = n - q * H;
    const float2 *col = w + q * M + pfboss_col(f0, q, j, M, H, L);
    float2 acc = make_float2(0.f, 0.f);
    for (long k = pfboss_k0(j, M, P, H, L); k < L; ++k) acc = mac<FUSED>(col[k * M], h[pfboss_tap(pfboss_offset(k, j, H, L), M, P)], acc);
    out[n] = acc;
}

hipError_t launch_pfb_os_synth_ola(const float2 *w, const float *h, float2 *out, long hops, int M, int P, long H, long f0, bool fused, hipStream_t st)
{
    if (hops <= 0) return hipSuccess;
    const long nout = hops * H, L = pfboss_L(M, P, H);
    const unsigned grid = (unsigned)((nout + 255) / 256);
    if (fused) hipLaunchKernelGGL(pfb_os_synth_ola_kernel<true>, dim3(grid), dim3(256), 0, st, w, h, out, nout, (long)M, (long)P, H, L, f0);
    else hipLaunchKernelGGL(pfb_os_synth_ola_kernel<false>, dim3(grid), dim3(256), 0, st, w, h, out, nout, (long)M, (long)P, H, L, f0);
    return hipGetLastError();
}

bool pfb_os_synth_supported(int nchan, int taps_per_branch, size_t hop)
{
    return nchan == PFB_M && hop == (size_t)PFBOS_H && (taps_per_branch == 4 || taps_per_branch == 8 || taps_per_branch == 16);
}

// x: hops + 2 P - 1 rows of 64 cf32; h: 64 P taps; tw64_inv: the 64-point INVERSE plan's table; out: 32 hops cf32 samples;
// first_row: F, of which only the parity matters at hop 32
hipError_t launch_pfb_os_synth(const float2 *x, const float *h, const float2 *tw64_inv, float2 *out, long hops, int taps_per_branch, uint64_t first_row,
                               bool fused, hipStream_t s)
{
    if (hops <= 0) return hipSuccess;
    const int fpar = (int)(first_row & 1);
    const long hpw = pfboss_hops_per_wave(hops), nwaves = pfboss_waves(hops);
    const unsigned grid = (unsigned)((nwaves + 3) / 4);
    const size_t lds = 4 * PFB_LDS * sizeof(float2);
    return pfb_wave_dispatch(taps_per_branch, fused, [&](auto p, auto f) {
        hipLaunchKernelGGL((pfb_os_synth64_kernel<decltype(p)::value, decltype(f)::value>), dim3(grid), dim3(256), lds, s, x, h, tw64_inv, out, hops, hpw, fpar);
        return hipGetLastError();
    });
}

} // namespace redio
