// pfb_os_kernels.hip -- 64-channel oversampled channelizer at hop 32 (include/redio.h, redio_pfb_os_*, route 1) on gfx950.
// Lane programs, index maps, launch geometry and the arithmetic contract: pfb_os_core.h.
//
// Algorithmic bytes: 8 B read from HBM + 16 B written per input sample (a row of 64 channels every 32 samples); 8 P + 60 flop per sample.
// Bound: HBM.  pfb64_kernel (pfb_kernels.hip) with two register windows: each wavefront owns a contiguous run of output rows, loads every
// half-row s_q (the 64 samples from 32 q on: 512 contiguous bytes per wave instruction) once, keeps the even-q and the odd-q window in
// registers from tile to tile and prefetches the next tile's half-rows while it computes.  Consecutive half-rows overlap by 256 bytes, so
// every 128-byte line of the stream is requested by two wave instructions of the same wavefront, sixteen apart at most in issue order:
// the second request is served by the compute unit's vector L1 (or by the XCD's L2 while the first is still in flight), not by HBM.
// No workgroup barrier: a wave's LDS tile is its own.
#include "fft_wave.h"
#include "pfb_wave.h"
#include "pfb_os_core.h"
#include "redio_internal.h"
#include <type_traits>

namespace redio {

// wide: `out` is 16-byte aligned (32-byte runs per lane as two 16-byte stores); otherwise four 8-byte stores
template <int P, bool FUSED>
__global__ __launch_bounds__(256) void pfb_os64_kernel(const float2 *__restrict__ x, const float *__restrict__ h, const float2 *__restrict__ tw,
                                                       float2 *__restrict__ out, long rows, long rows_per_wave, int fpar, int wide)
{
    static_assert(PFB_TILE % P == 0, "two tiles move a parity's window by 16 slots: it rotates in place only if P divides 16");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *lds = reinterpret_cast<float2 *>(smem) + wave * PFB_LDS;
    const long t0 = ((long)blockIdx.x * 4 + wave) * rows_per_wave;
    if (t0 >= rows) return; // wave-uniform; no workgroup barrier in this kernel
    const long t1 = (t0 + rows_per_wave < rows) ? t0 + rows_per_wave : rows;

    float g[P];
#pragma unroll
    for (int p = 0; p < P; ++p) g[p] = h[PFB_M * p + lane];
    // ONE straight-line path, as pfb64_kernel's load_rows: a half-row past the end of the stream (only the last tiles of the last wave
    // ever ask for one) is clamped with scalar arithmetic and a tile's request is never skipped, so the compiler can count the loads in
    // flight at every use
    auto load_halves = [&](float2(&dst)[PFB_TILE], long first) {
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) dst[ti] = x[PFBOS_H * pfbos_half(first + ti, rows, P) + (unsigned)lane];
    };
    // the transform's twiddles, once per wavefront (pfb_core.h: why not inside the tile loop): 20 scalar and 24 vector registers
    PFB_WAVE_TWIDDLES(tw, lane);
    // exchange 1's store lane of even and of odd tile rows: the shift s_r = 32 ((F + r) & 1), folded into the index
    const int lane_ev = pfbos_x1_lane(lane, 0, fpar), lane_od = pfbos_x1_lane(lane, 1, fpar);
    // the two windows: win[par][slot], taps 0 .. P - 2 of the run's first row of each parity (never past the stream: t0 + 2 P - 3 < rows + 2 P - 3)
    float2 win[2][P];
#pragma unroll
    for (int p = 0; p < P - 1; ++p)
#pragma unroll
        for (int par = 0; par < 2; ++par) win[par][pfbos_slot(0, p, P)] = x[PFBOS_H * (t0 + par + 2 * p) + (unsigned)lane];
    // One tile: rows tb .. tb + 15, whose entering half-rows are in `cur`; the next tile's are requested into `nx` before the arithmetic.
    // The tile loop is unrolled by two with the roles of the two register sets swapped (pfb64_kernel: why); a tile moves each window by
    // 8 slots, so the second tile of the pair starts at J0 = 8 -- every slot index is a compile-time constant at all three P.
    auto tile = [&](long tb, auto j0, float2(&cur)[PFB_TILE], float2(&nx)[PFB_TILE]) {
        constexpr int J0 = decltype(j0)::value;
        load_halves(nx, pfbos_enter(tb + PFB_TILE, P));
        // branch FIRs: lane = branch, strict fold over p (dsputils.rs:31)
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) {
            const int par = ti & 1, j = J0 + (ti >> 1);
            win[par][pfbos_slot(j, P - 1, P)] = cur[ti];
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int p = 0; p < P; ++p) acc = mac<FUSED>(win[par][pfbos_slot(j, p, P)], g[p], acc);
            lds[pfb_x1_store(ti, par ? lane_od : lane_ev)] = acc;
        }
        wave_lds_fence();
        float2 v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) v[e] = lds[pfb_x1_load(lane, e)];
        wave_lds_fence();
        pfb_fft64_passAB_pre<false>(v, twone, twa1, twa2, twa3);
#pragma unroll
        for (int k2 = 0; k2 < 4; ++k2)
#pragma unroll
            for (int k1 = 0; k1 < 4; ++k1) lds[pfb_x2_store(lane, k1, k2)] = v[k1 + 4 * k2];
        wave_lds_fence();
#pragma unroll
        for (int f = 0; f < 16; ++f) v[f] = lds[pfb_x2_load(lane, f)];
        wave_lds_fence();
        pfb_fft64_passC_pre<false>(v, twc1, twc2, twc3);
        const long row = tb + (lane >> 2);
        if (row < t1) { // channels 16 k0 + 4 (lane & 3) + k2 of row tb + (lane >> 2): 32 bytes per lane, 128 per row and k0
            float2 *orow = out + PFB_M * tb + (unsigned)(PFB_M * (lane >> 2) + 4 * (lane & 3));
            if (wide) {
#pragma unroll
                for (int k0 = 0; k0 < 4; ++k0) {
                    *reinterpret_cast<float4 *>(orow + 16 * k0) = make_float4(v[k0].x, v[k0].y, v[k0 + 4].x, v[k0 + 4].y);
                    *reinterpret_cast<float4 *>(orow + 16 * k0 + 2) = make_float4(v[k0 + 8].x, v[k0 + 8].y, v[k0 + 12].x, v[k0 + 12].y);
                }
            } else {
#pragma unroll
                for (int k0 = 0; k0 < 4; ++k0)
#pragma unroll
                    for (int k2 = 0; k2 < 4; ++k2) orow[16 * k0 + k2] = v[k0 + 4 * k2];
            }
        }
    };
    float2 ra[PFB_TILE], rb[PFB_TILE];
    load_halves(ra, pfbos_enter(t0, P));
    for (long tb = t0; tb < t1; tb += 2 * PFB_TILE) {
        tile(tb, std::integral_constant<int, 0>{}, ra, rb);
        if (tb + PFB_TILE < t1) tile(tb + PFB_TILE, std::integral_constant<int, PFB_TILE / 2>{}, rb, ra);
    }
}

bool pfb_os_supported(int nchan, int taps_per_branch, size_t hop)
{
    return nchan == PFB_M && hop == (size_t)PFBOS_H && (taps_per_branch == 4 || taps_per_branch == 8 || taps_per_branch == 16);
}

// x: 32 (rows - 1) + 64 P cf32 samples; h: 64 P taps; tw64: the 64-point forward plan's table; out: rows rows of 64 cf32;
// first_row: F, of which only the parity matters at hop 32
hipError_t launch_pfb_os(const float2 *x, const float *h, const float2 *tw64, float2 *out, long rows, int taps_per_branch, uint64_t first_row, bool fused,
                         hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    const int fpar = (int)(first_row & 1);
    const long rpw = pfbos_rows_per_wave(rows), nwaves = pfbos_waves(rows);
    const unsigned grid = (unsigned)((nwaves + 3) / 4);
    const size_t lds = 4 * PFB_LDS * sizeof(float2);
    const int wide = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    return pfb_wave_dispatch(taps_per_branch, fused, [&](auto p, auto f) {
        hipLaunchKernelGGL((pfb_os64_kernel<decltype(p)::value, decltype(f)::value>), dim3(grid), dim3(256), lds, s, x, h, tw64, out, rows, rpw, fpar, wide);
        return hipGetLastError();
    });
}

// Route 0's first pass: pfb_branch_kernel (pfb_api.hip) with a row stride of H: v[r][(m + s_r) mod M] = fold_p x[r H + p M + m] * h[M p + m]
// (ascending p, the reference's fold).  Rows H apart share samples only where H divides a multiple of M, so a thread is one (row, branch)
// and walks its P taps; consecutive threads are consecutive m (coalesced loads; the store is two coalesced runs, split where the rotation
// wraps).  f0 = (F + the pass's first row) mod M.
template <bool FUSED>
__global__ __launch_bounds__(256) void pfb_os_branch_kernel(const float2 *__restrict__ x, const float *__restrict__ h, float2 *__restrict__ v, long rows,
                                                            int M, int P, long H, long f0)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * M) return;
    const long r = e / M;
    const int m = (int)(e - r * M);
    const float2 *col = x + r * H + m;
    float2 acc = make_float2(0.f, 0.f);
    for (int p = 0; p < P; ++p) acc = mac<FUSED>(col[(long)p * M], h[(long)p * M + m], acc);
    v[r * M + pfbos_rot(m, pfbos_shift(f0, r, M, H), M)] = acc;
}

__attribute__((visibility("hidden"))) // library-internal: not in the exported symbol set
hipError_t launch_pfb_os_branch(const float2 *x, const float *h, float2 *v, long rows, int M, int P, long H, long f0, bool fused, hipStream_t st)
{
    if (rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((rows * M + 255) / 256);
    if (fused) hipLaunchKernelGGL(pfb_os_branch_kernel<true>, dim3(grid), dim3(256), 0, st, x, h, v, rows, M, P, H, f0);
    else hipLaunchKernelGGL(pfb_os_branch_kernel<false>, dim3(grid), dim3(256), 0, st, x, h, v, rows, M, P, H, f0);
    return hipGetLastError();
}

} // namespace redio
