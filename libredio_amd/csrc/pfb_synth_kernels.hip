// pfb_synth_kernels.hip -- 64-channel synthesis filterbank (include/redio.h, redio_pfb_synth_*, route 1) on gfx950.
// Lane programs, index maps, launch geometry and the arithmetic contract: pfb_synth_core.h.
//
// Algorithmic bytes: 8 B read + 8 B written per sample, the channelizer's traffic; 4 P + 30 flop per sample (+ the halo's transforms: one
// tile per wave, at most 15 / 64 extra at the smallest run).  Bound: HBM.  pfb64_kernel (pfb_kernels.hip) run the other way round: each
// wavefront owns a contiguous run of OUTPUT rows, walks the input rows of that run and its P - 1 rows of halo in tiles of 16, loads every
// row once as 512 contiguous bytes per wave instruction (lane = channel; rows reach the transform's lane layout through the padded LDS tile
// -- the other form, 32-byte runs per lane straight into that layout, spreads one wave instruction over sixteen rows' lines and cannot be
// clamped per row with scalar arithmetic), keeps the filter window in registers from tile to tile, and stores one output row per wave
// instruction.  No workgroup barrier: a wave's LDS tile is its own.
#include "fft_wave.h"
#include "pfb_wave.h"
#include "pfb_synth_core.h"
#include "redio_internal.h"

namespace redio {

template <int P, bool FUSED>
__global__ __launch_bounds__(256) void pfb_synth64_kernel(const float2 *__restrict__ x, const float *__restrict__ h, const float2 *__restrict__ tw,
                                                          float2 *__restrict__ out, long rows, long rows_per_wave)
{
    static_assert(PFB_TILE % P == 0, "the register window rotates in place only if the tile is a multiple of P");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *lds = reinterpret_cast<float2 *>(smem) + wave * PFB_LDS;
    const long t0 = ((long)blockIdx.x * 4 + wave) * rows_per_wave; // output rows [t0, t1)
    if (t0 >= rows) return; // wave-uniform; no workgroup barrier in this kernel
    const long t1 = (t0 + rows_per_wave < rows) ? t0 + rows_per_wave : rows;
    const long r_end = t1 + P - 1; // input rows [t0, r_end)

    float g[P];
#pragma unroll
    for (int p = 0; p < P; ++p) g[p] = h[PFB_M * p + lane];
    // ONE straight-line path, as pfb64_kernel's load_rows: a row past the end of the stream is clamped with scalar arithmetic and a tile's
    // request is never skipped, so the compiler can count the loads in flight at every use
    auto load_rows = [&](float2(&dst)[PFB_TILE], long first) {
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) dst[ti] = x[PFB_M * pfbs_in_row(first + ti, rows, P) + (unsigned)lane];
    };
    // the inverse transform's twiddles, once per wavefront (pfb_core.h: why not inside the tile loop): 20 scalar and 24 vector registers
    PFB_WAVE_TWIDDLES(tw, lane);
    float2 win[P];
#pragma unroll
    for (int p = 0; p < P; ++p) win[p] = make_float2(0.f, 0.f); // the halo's outputs are never stored: any finite start will do
    // One tile: input rows rb .. rb + 15 from `cur`, the next tile's rows requested into `nx` before the arithmetic (pfb64_kernel's cf32 form;
    // the tile loop is unrolled by two with the roles of the two register sets swapped, for the reason written there).
    auto tile = [&](long rb, float2(&cur)[PFB_TILE], float2(&nx)[PFB_TILE]) {
        load_rows(nx, rb + PFB_TILE);
        // exchange 1: lane = channel -> the transform's layout
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) lds[pfb_x1_store(ti, lane)] = cur[ti];
        wave_lds_fence();
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
        // exchange 3: lane (tt, k1) holding X[k2 + 4 k1 + 16 k0] -> lane = branch
#pragma unroll
        for (int k0 = 0; k0 < 4; ++k0)
#pragma unroll
            for (int k2 = 0; k2 < 4; ++k2) lds[pfbs_x3_store(lane, k0, k2)] = v[k0 + 4 * k2];
        wave_lds_fence();
        // branch FIRs: lane = branch, strict fold over p (dsputils.rs:31); input row rb + ti completes output row rb + ti - (P - 1)
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) {
            win[(ti + P - 1) % P] = lds[pfbs_x3_load(ti, lane)];
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int p = 0; p < P; ++p) acc = mac<FUSED>(win[(ti + p) % P], g[p], acc);
            if (pfbs_stores(rb + ti, t0, t1, P)) out[PFB_M * (rb + ti - (P - 1)) + (unsigned)lane] = acc; // wave-uniform: 512 bytes per instruction
        }
        wave_lds_fence(); // the next tile's exchange 1 overwrites what the filters have just read
    };
    float2 ra[PFB_TILE], rb2[PFB_TILE];
    load_rows(ra, t0);
    for (long rb = t0; rb < r_end; rb += 2 * PFB_TILE) {
        tile(rb, ra, rb2);
        if (rb + PFB_TILE < r_end) tile(rb + PFB_TILE, rb2, ra);
    }
}

bool pfb_synth_supported(int nchan, int taps_per_branch)
{
    return nchan == PFB_M && (taps_per_branch == 4 || taps_per_branch == 8 || taps_per_branch == 16);
}

// x: rows + P - 1 rows of 64 cf32; h: 64 P taps; tw64_inv: the 64-point INVERSE plan's table; out: rows rows of 64 cf32
hipError_t launch_pfb_synth(const float2 *x, const float *h, const float2 *tw64_inv, float2 *out, long rows, int taps_per_branch, bool fused, hipStream_t s)
{
    if (rows <= 0) return hipSuccess;
    const long rpw = pfbs_rows_per_wave(rows), nwaves = pfbs_waves(rows);
    const unsigned grid = (unsigned)((nwaves + 3) / 4);
    const size_t lds = 4 * PFB_LDS * sizeof(float2);
    return pfb_wave_dispatch(taps_per_branch, fused, [&](auto p, auto f) {
        hipLaunchKernelGGL((pfb_synth64_kernel<decltype(p)::value, decltype(f)::value>), dim3(grid), dim3(256), lds, s, x, h, tw64_inv, out, rows, rpw);
        return hipGetLastError();
    });
}

} // namespace redio
