// pfb_pspec_kernels.hip -- the fused 64-channel polyphase spectrometer (redio_pfb_pspec_*; contract: DESIGN.md 5.6b) on gfx950.
// Lane programs: pfb_core.h (the channelizer's rows), pfb_pspec_core.h (the power tile and the fold).
//
// Algorithmic bytes: 8 B (cf32) or 2 B (u8 I/Q) read per input sample + 4 / K written; 4 P + 30 + 3 flop per sample.
// Bound: HBM from cf32 (the channelizer's kernel without its 8 B per sample of stores), VALU from bytes.
// pfbspec64_kernel is pfb64_kernel (pfb_kernels.hip) up to the end of the transform: the register window, the two LDS exchanges,
// the twiddles kept in registers, the prefetch.  Then, instead of storing the tile's rows, the wave squares them into a 16 x 64
// f32 tile in its own LDS region, and lane = channel folds the tile's rows, in ascending order, into the sums of DESIGN.md 5.3c.
// A sibling and not a template parameter of pfb64_kernel: that kernel keeps its name and its code.
#include "fft_wave.h"
#include "pfb_wave.h"
#include "pfb_pspec_core.h"
#include <type_traits>
#include "redio_internal.h"

namespace redio {

// A wave owns units [u0, u1) of the launch -- whole output rows, or with `split` whole segments (pspec_unit) -- which are the
// consecutive channelizer rows [t0, t1); `rows` = every channelizer row the launch sums (the input holds rows + P - 1 rows of samples).
// dst: 64 f32 per unit (the output rows, or the segment partials).  IN_U8: x is the receiver's interleaved u8 I/Q bytes, a 2-byte
// load per sample, requested after the branch filters as in pfb64_kernel<.., IN_U8 = 1>.
template <int P, bool FUSED, int IN_U8>
__global__ __launch_bounds__(256) void pfbspec64_kernel(const float2 *__restrict__ x, const float *__restrict__ h,
                                                        const float2 *__restrict__ tw, float *__restrict__ dst, long rows, long nunits,
                                                        long units_per_wave, long K, int split)
{
    static_assert(PFB_TILE % P == 0, "the register window rotates in place only if the tile is a multiple of P");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    float2 *lds = reinterpret_cast<float2 *>(smem) + wave * PFB_LDS;
    float *pt = reinterpret_cast<float *>(lds); // the power tile, in the same region
    const long u0 = ((long)blockIdx.x * 4 + wave) * units_per_wave;
    if (u0 >= nunits) return; // wave-uniform; no workgroup barrier in this kernel
    const long u1 = (u0 + units_per_wave < nunits) ? u0 + units_per_wave : nunits;
    PfbSpecFold fold;
    long t0;
    pfbspec_fold_begin(fold, u0, K, split != 0, t0);
    const long t1 = pfbspec_units_end(u1, K, split != 0);
    const long last_in_row = rows + P - 2; // the last row of samples the launch may read

    float g[P];
#pragma unroll
    for (int p = 0; p < P; ++p) g[p] = h[PFB_M * p + lane];
    using raw_t = typename std::conditional<IN_U8 != 0, unsigned short, float2>::type; // one sample as it lies in memory
    const raw_t *xraw = reinterpret_cast<const raw_t *>(x);
    auto ld = [](const raw_t *p) -> raw_t {
        if constexpr (IN_U8 != 0) return __builtin_nontemporal_load(p); // read once; the policy pfb64_kernel measured for bytes
        else return *p;
    };
    auto sample = [](raw_t w) -> float2 {
        if constexpr (IN_U8 != 0) return make_float2(i2f(w & 255u), i2f((unsigned)w >> 8));
        else return w;
    };
    // one straight-line path, rows past the end of the stream clamped with scalar arithmetic, a tile's request never skipped
    // (pfb64_kernel: why)
    auto load_rows = [&](raw_t(&dst_rows)[PFB_TILE], long first) {
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) {
            long r = first + ti;
            r = r < last_in_row ? r : last_in_row;
            dst_rows[ti] = ld(xraw + PFB_M * r + (unsigned)lane);
        }
    };
    PFB_WAVE_TWIDDLES(tw, lane);
    float2 win[P];
#pragma unroll
    for (int p = 0; p < P - 1; ++p) win[p] = sample(ld(xraw + PFB_M * (t0 + p) + (unsigned)lane));
    float seg = 0.f, row = 0.f; // this lane's channel: the segment and the output row being summed
    constexpr bool LATE = IN_U8 != 0;
    auto tile = [&](long tb, raw_t(&cur)[PFB_TILE], raw_t(&nx)[PFB_TILE]) {
        if (!LATE) load_rows(nx, tb + PFB_TILE + P - 1);
        // branch FIRs: lane = branch, strict fold over p (dsputils.rs:31)
#pragma unroll
        for (int ti = 0; ti < PFB_TILE; ++ti) {
            win[(ti + P - 1) % P] = sample(cur[ti]);
            float2 acc = make_float2(0.f, 0.f);
#pragma unroll
            for (int p = 0; p < P; ++p) acc = mac<FUSED>(win[(ti + p) % P], g[p], acc);
            lds[pfb_x1_store(ti, lane)] = acc;
        }
        if (LATE) load_rows(cur, tb + PFB_TILE + P - 1); // into the registers the branch filters have just emptied
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
        // the power tile: lane (tt, k1) writes four 16-byte runs of row tt, then lane = channel reads one word of every row
#pragma unroll
        for (int k0 = 0; k0 < 4; ++k0)
            *reinterpret_cast<float4 *>(pt + pfbspec_tile_index(lane >> 2, pfb_out_channel(lane, k0, 0))) = pfbspec_power4(v, k0);
        wave_lds_fence();
        float pw[PFB_TILE];
#pragma unroll
        for (int tt = 0; tt < PFB_TILE; ++tt) pw[tt] = pt[pfbspec_tile_index(tt, lane)];
        wave_lds_fence(); // before the next tile's branch filters write the region
#pragma unroll
        for (int tt = 0; tt < PFB_TILE; ++tt)
            if (tb + tt < t1) pfbspec_fold_step(fold, pw[tt], seg, row, K, split != 0, dst, lane); // wave-uniform
    };
    raw_t ra[PFB_TILE], rb[PFB_TILE];
    load_rows(ra, t0 + P - 1);
    for (long tb = t0; tb < t1; tb += 2 * PFB_TILE) {
        if constexpr (LATE) { // one register set
            tile(tb, ra, ra);
            if (tb + PFB_TILE < t1) tile(tb + PFB_TILE, ra, ra);
        } else {
            tile(tb, ra, rb);
            if (tb + PFB_TILE < t1) tile(tb + PFB_TILE, rb, ra);
        }
    }
}

template <int P, int IN_U8>
static hipError_t launch_pfbspec_t(const void *x, const float *h, const float2 *tw, float *dst, long nunits, long K, bool split, bool fused,
                                   hipStream_t s)
{
    const long S = pspec_nseg(K);
    const long rows = (split ? nunits / S : nunits) * K; // a launch holds whole output rows
    const long upw = pfbspec_units_per_wave(nunits, K, split);
    const long nwaves = (nunits + upw - 1) / upw;
    const long grid = (nwaves + 3) / 4;
    if (grid > 0x7fffffffl) return hipErrorInvalidValue;
    const size_t lds = 4 * PFB_LDS * sizeof(float2);
    if (fused)
        hipLaunchKernelGGL((pfbspec64_kernel<P, true, IN_U8>), dim3((unsigned)grid), dim3(256), lds, s, (const float2 *)x, h, tw, dst, rows, nunits, upw,
                           K, split ? 1 : 0);
    else
        hipLaunchKernelGGL((pfbspec64_kernel<P, false, IN_U8>), dim3((unsigned)grid), dim3(256), lds, s, (const float2 *)x, h, tw, dst, rows, nunits, upw,
                           K, split ? 1 : 0);
    return hipGetLastError();
}

// x: cf32 samples (8-byte aligned) or, with in_u8, u8 I/Q byte pairs (2-byte aligned); nunits: output rows, or with `split` their
// segments (a whole number of rows' worth); dst: 64 f32 per unit
hipError_t launch_pfbspec64(const void *x, bool in_u8, const float *h, const float2 *tw64, float *dst, long nunits, long K, int taps_per_branch,
                            bool split, bool fused, hipStream_t s)
{
    if (nunits <= 0) return hipSuccess;
    switch (taps_per_branch) {
    case 16: return in_u8 ? launch_pfbspec_t<16, 1>(x, h, tw64, dst, nunits, K, split, fused, s) : launch_pfbspec_t<16, 0>(x, h, tw64, dst, nunits, K, split, fused, s);
    case 8: return in_u8 ? launch_pfbspec_t<8, 1>(x, h, tw64, dst, nunits, K, split, fused, s) : launch_pfbspec_t<8, 0>(x, h, tw64, dst, nunits, K, split, fused, s);
    case 4: return in_u8 ? launch_pfbspec_t<4, 1>(x, h, tw64, dst, nunits, K, split, fused, s) : launch_pfbspec_t<4, 0>(x, h, tw64, dst, nunits, K, split, fused, s);
    default: return hipErrorNotSupported;
    }
}

} // namespace redio
