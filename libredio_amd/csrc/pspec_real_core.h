// pspec_real_core.h -- the real-input integrated power spectrum (redio_pspec_real_*; contract: DESIGN.md 5.3d): the lane programs of
// the fused 2048-point kernel around the one-wave transform of fft_core.h and the split step of fftr_core.h, and the thread program
// of the generic row gather.  The summation order, the accumulate and the fold thread programs are pspec_core.h's, with a row of
// B = N / 2 + 1 bins.  Every multiply and add is rounded on its own.
//
//     X      = kiss_fftr(x w)                       the complex transform of size M = N / 2, then the published split loop
//     p_t[k] = X[k].re * X[k].re + X[k].im * X[k].im       k = 0 ... M
//
// Host-compilable (tests/emu_pspec_real runs the same programs on the CPU).
#pragma once
#include "fftr_core.h"
#include "pspec_core.h"

namespace redio {

constexpr int PSPECR2K_B = FFTR1K_M + 1; // bins of the fused size: a row of the output, or a segment's partial

// Auto mode (redio_pspec_real_set_split(h, 0)) gives a wave one SEGMENT instead of one whole row when K > PSPEC_SEG and the call has
// fewer rows than this.  The real plan's own constant.
constexpr long PSPEC_REAL_SPLIT_ROWS = 2048;

// ---- the fused 2048-point kernel's lane programs.  The real row is M = 1024 cf32: v[t] = (x[2 e], x[2 e + 1]), e = lane + 64 t
// (fft1k_passA's layout).  PAIRS: the row is 8-byte aligned and is read as float2 (xp: float2 elements); otherwise as two floats.
template <typename X2Ptr>
RD_HD void pspecr2k_load_pairs(float2 (&v)[16], X2Ptr xp, int lane)
{
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = xp[lane + 64 * t];
}
template <typename XPtr>
RD_HD void pspecr2k_load_singles(float2 (&v)[16], XPtr x, int lane)
{
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int e = lane + 64 * t;
        v[t] = make_float2(x[2 * e], x[2 * e + 1]);
    }
}
// the lane's window values as pairs: w[t] = (win[2 e], win[2 e + 1])
template <typename WPtr>
RD_HD void pspecr2k_load_window(float2 (&w)[16], WPtr win, int lane)
{
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int e = lane + 64 * t;
        w[t] = make_float2(win[2 * e], win[2 * e + 1]);
    }
}
RD_HD void pspecr2k_window(float2 (&v)[16], const float2 (&w)[16])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = make_float2(mul_rn(v[t].x, w[t].x), mul_rn(v[t].y, w[t].y));
}
// Z in natural order into the wave's LDS image: after fft1k_passC v[4 q + j] = Z[lane + 64 q + 256 j]
template <typename ExPtr>
RD_HD void pspecr2k_image(const float2 (&v)[16], ExPtr ex, int lane)
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) ex[lane + 64 * q + 256 * j] = v[4 * q + j];
}
// the split step of fftr1k_post_lane_regs with each pair squared as it is produced: p[t] = |X[k]|^2, p[8 + t] = |X[1024 - k]|^2
// (k = lane + 64 t, t < 8; lane 0's t = 0 is the DC / Nyquist pair), p[16] = |X[512]|^2 (lane 0; the other lanes never store theirs)
template <typename ExPtr>
RD_HD void pspecr2k_split_power(const float2 (&v)[16], ExPtr ex, const Fftr1kTw &w, int lane, float (&p)[17])
{
    float2 lo, hi;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float2 zk = v[fftr1k_reg(t)];
        if (t == 0 && lane == 0) {
            fftr_fwd_ends(zk, lo, hi);
        } else {
            const float2 zm = ex[fftr1k_partner(lane, t)];
            fftr_fwd_pair(zk, zm, w.s[t], lo, hi);
        }
        p[t] = pspec_power(lo);
        p[8 + t] = pspec_power(hi);
    }
    p[16] = 0.f;
    if (lane == 0) {
        const float2 z = v[fftr1k_reg(8)];
        fftr_fwd_pair(z, z, w.mid, lo, hi);
        p[16] = pspec_power(hi);
    }
}
RD_HD void pspecr2k_accum(const float (&p)[17], float (&seg)[17], bool first)
{
    if (first) {
#pragma unroll
        for (int i = 0; i < 17; ++i) seg[i] = p[i];
    } else {
#pragma unroll
        for (int i = 0; i < 17; ++i) seg[i] = add_rn(seg[i], p[i]);
    }
}
RD_HD void pspecr2k_fold(const float (&seg)[17], float (&row)[17], bool first) { pspec_fold_regs(seg, row, first); }
// dst: the unit's 1025 f32 (a row of the output, or a segment's partial; only 4-byte aligned): eight ascending and eight descending
// wave-wide stores and lane 0's bin 512 -- every element once
template <typename OutPtr>
RD_HD void pspecr2k_store(const float (&row)[17], OutPtr dst, int lane)
{
#pragma unroll
    for (int t = 0; t < 8; ++t) dst[lane + 64 * t] = row[t];
#pragma unroll
    for (int t = 0; t < 8; ++t) dst[fftr1k_partner(lane, t)] = row[8 + t];
    if (lane == 0) dst[FFTR1K_M / 2] = row[16];
}

// ---- the generic path's row gather: element n of packed row b = x[b step + n], times win[n] when there is a window
template <typename XPtr, typename WPtr>
RD_HD float pspec_real_rows_thread(XPtr x, WPtr win, bool windowed, long b, long n, long step)
{
    const float v = x[b * step + n];
    return windowed ? mul_rn(v, win[n]) : v;
}

} // namespace redio
