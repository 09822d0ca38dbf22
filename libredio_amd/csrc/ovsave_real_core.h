// ovsave_real_core.h -- the lane programs of the fused 2048-point real overlap-save block that are not already in fftr_core.h: the
// product with conj(H) on the split's register layout, and the masked, scaled store of the block's hop outputs.  Every multiply
// and add is rounded on its own.
//
// Host-compilable (tests/emu_ovsave_real runs the same lane programs on the CPU).
#pragma once
#include "fftr_core.h"

namespace redio {

// Y = X .* Hc on the layout of fftr1k_post_lane_regs / fftr1k_load_row: a[t] = bin k, b[t] = bin 1024 - k (k = lane + 64 t),
// mid = bin 512.  Hc: the 1025 bins of conj(kiss_fftr(padded taps)).
template <typename HcPtr>
RD_HD void ovsr1k_product(float2 (&a)[8], float2 (&b)[8], float2 &mid, HcPtr Hc, int lane)
{
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = lane + 64 * t;
        a[t] = cmul_rn(a[t], Hc[k]);
        b[t] = cmul_rn(b[t], Hc[FFTR1K_M - k]);
    }
    mid = cmul_rn(mid, Hc[FFTR1K_M / 2]);
}

// v: the inverse transform's result registers (v[4 q + j] = the real pair 2 p, 2 p + 1 with p = lane + 64 q + 256 j); out: the
// block's outputs as pairs.  hop is even, so a pair lies wholly inside or wholly outside [0, hop).
template <typename OutPtr>
RD_HD void ovsr1k_store(const float2 (&v)[16], OutPtr out, int lane, long hop, float scale)
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int p = lane + 64 * q + 256 * j;
            if (2 * (long)p < hop) out[p] = make_float2(mul_rn(v[4 * q + j].x, scale), mul_rn(v[4 * q + j].y, scale));
        }
}

} // namespace redio
