// ddc_upfirdn_core.h -- the tuned resampler (include/redio.h, redio_ddc_upfirdn_*): the tuner's oscillator mix in front of the rational
// resampler, in one kernel.
//
// Arithmetic contract: kpn::mul_vecs (src/kpn/src/kpn.rs:198-203) with a periodic constant vector, then the resampler's polyphase form of
// dsputils::convolve (src/dsputils/src/dsputils.rs:30-32):
//   m[n] = cmul_rn(x[n], w[(first + n) mod L])     ddc_core.h's mix: every operation rounded on its own, never contracted
//   y    = upfirdn_core.h's contract over m         (stuffed zeros skipped; FUSED selects fmaf for the fold only)
// so every output is bit-equal to redio_upfirdn_enqueue (complex) on redio_mul_c32(x, the table tiled from first).  The u8 entry
// converts each byte with i2f (redio_device.h) first.
//
// Route 1 is the resampler's tiled kernel body with the tuner's loader as its policy (upfirdn_tile_kernels.h, DdcTile): a workgroup takes
// the tuner's one modulo for its tile's first sample, base = (first + t * 256 R D') mod L, and its lanes read table entries
// base + n, n < tile_in + 2.  The image is at most UPFIRDN_LDS_MAX / 8 cf32, so that index stays inside the extended table
// (asserted below).  Route 2 is one output per thread, any U, D and K: upfirdn_direct_output's walk with the mix in it, one 64-bit modulo per
// thread for the window's first sample, then wrap by compare as ddc_direct_output does.
//
// Host-compilable (tests/emu_ddc_upfirdn runs every thread of a call on the CPU).
#pragma once
#include "ddc_core.h"
#include "upfirdn_core.h"

namespace redio {

// a lane of route 1 reads table entry base + n for n < tile_in + 2, and no image that route 1 stages is larger than the LDS budget
static_assert(UPFIRDN_LDS_MAX / 8 + 2 <= DDC_TABLE_EXT, "a lane's table index stays inside the extended table for every tile route 1 takes");
// the same as a condition on one shape (the launcher checks it next to the launch; tile_in <= image elements <= UPFIRDN_LDS_MAX / 8)
RD_HD constexpr bool ddc_upfirdn_tile_ok(int R, long Dp, long Wp) { return upfirdn_tile_in(R, Dp, Wp) + 2 <= DDC_TABLE_EXT; }

// route 2, output i of a call.  x: the call's first sample (cf32, or with U8 its first byte: two bytes per sample); first_mod =
// first_index mod L; tab: the table (L entries are enough here: the index wraps by compare)
template <bool U8, bool FUSED>
RD_HD float2 ddc_upfirdn_direct_output(const void *x, long i, long Up, long Dp, const UpfirdnPhase *__restrict__ ph, const float *__restrict__ taps,
                                       unsigned first_mod, const float2 *__restrict__ tab, unsigned L)
{
    const long q = i / Up;
    const UpfirdnPhase p = ph[i - q * Up];
    const long n0 = q * Dp + p.s; // the window's first sample
    const float2 *xc = reinterpret_cast<const float2 *>(x) + n0;
    const unsigned char *xb = reinterpret_cast<const unsigned char *>(x) + 2 * n0;
    const float *g = taps + p.off;
    unsigned idx = ddc_base(first_mod, (unsigned long long)n0, L); // (first + q D' + s(r)) mod L: the thread's one modulo
    float2 acc = make_float2(0.f, 0.f);
    for (int t = 0; t < p.k; ++t) {
        float2 m;
        if constexpr (U8) m = ddc_mix_u8(xb[2 * t], xb[2 * t + 1], tab[idx]);
        else m = cmul_rn(xc[t], tab[idx]);
        acc = mac<FUSED>(m, g[t], acc);
        if (++idx == L) idx = 0;
    }
    return acc;
}

} // namespace redio
