// pspec_core.h -- the integrated power spectrum (redio_pspec_*; contract: DESIGN.md 5.3c): the summation order, the lane programs of
// the fused 1024-point kernel around the one-wave transform of fft_core.h, and the thread programs of the generic accumulate and
// fold passes.  Every multiply and add is rounded on its own.
//
//     p_t[k]    = X_t[k].re * X_t[k].re + X_t[k].im * X_t[k].im
//     seg_s[k]  = ((p_16s + p_16s+1) + ...)         t in [16 s, min(16 s + 16, K)), a left fold that starts from its first term
//     out[r][k] = ((seg_0 + seg_1) + ...)           a left fold in ascending s
//
// Host-compilable (tests/emu_pspec and tests/emu_pspec_u8 run the same programs on the CPU).
#pragma once
#include "fft_core.h"

namespace redio {

constexpr int PSPEC_SEG = 16; // REDIO_PSPEC_SEG of include/redio.h: transforms per segment of the blocked sum

// Auto mode (redio_pspec_set_split(h, 0)) gives a wave one SEGMENT instead of one whole row when K > PSPEC_SEG and the call has
// fewer rows than this.  Set from a measurement (2^28 samples, K = 32 ... 1024 in both modes): a wave per row is
// ahead by 4-8 % from 2048 rows up, a wave per segment by 8 % at 1024 rows, 1.8 x at 512 and 3.7 x at 256.  The first guess was
// 4096 = 256 CUs x 4 SIMDs x 4 waves.
constexpr long PSPEC_SPLIT_ROWS = 2048;

RD_HD float pspec_power(float2 X) { return add_rn(mul_rn(X.x, X.x), mul_rn(X.y, X.y)); }

RD_HD long pspec_nseg(long K) { return (K + PSPEC_SEG - 1) / PSPEC_SEG; }

// segment q of a call (q = row * S + s, S = pspec_nseg(K)): its first transform, counted from the call's first, and how many it holds
RD_HD void pspec_segment(long q, long K, long S, long &g, long &cnt)
{
    const long r = q / S, s = q - r * S;
    g = r * K + (long)PSPEC_SEG * s;
    cnt = K - (long)PSPEC_SEG * s < PSPEC_SEG ? K - (long)PSPEC_SEG * s : PSPEC_SEG;
}

// unit u of a fused launch: a whole row (split == false: transforms [0, K) of row u) or one segment (unit u = segment u)
RD_HD void pspec_unit(long u, long K, bool split, long &g0, long &cnt)
{
    if (split) {
        pspec_segment(u, K, pspec_nseg(K), g0, cnt);
    } else {
        g0 = u * K;
        cnt = K;
    }
}

// what transform i (0 ... cnt - 1) of a unit does to the two accumulators
struct PspecStep {
    bool seg_first; // the segment accumulator is assigned, not added to
    bool seg_last;  // the segment folds into the row accumulator after this transform
    bool row_first; // ... by assignment: it is the unit's first segment
};
RD_HD PspecStep pspec_step(long i, long cnt)
{
    PspecStep s;
    s.seg_first = i % PSPEC_SEG == 0;
    s.seg_last = i % PSPEC_SEG == PSPEC_SEG - 1 || i + 1 == cnt;
    s.row_first = i < PSPEC_SEG;
    return s;
}

// ---- the fused 1024-point kernel's lane programs: v[t] = x[lane + 64 t] on the way in (fft1k_passA's layout), and after
// fft1k_passC v[4 q + j] = X[lane + 64 q + 256 j]
template <typename XPtr>
RD_HD void pspec1k_load(float2 (&v)[16], XPtr x, int lane)
{
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = x[lane + 64 * t];
}
template <typename WPtr>
RD_HD void pspec1k_load_window(float (&w)[16], WPtr win, int lane)
{
#pragma unroll
    for (int t = 0; t < 16; ++t) w[t] = win[lane + 64 * t];
}
RD_HD void pspec1k_window(float2 (&v)[16], const float (&w)[16])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = make_float2(mul_rn(v[t].x, w[t]), mul_rn(v[t].y, w[t]));
}
RD_HD void pspec1k_accum(const float2 (&v)[16], float (&seg)[16], bool first)
{
    if (first) {
#pragma unroll
        for (int i = 0; i < 16; ++i) seg[i] = pspec_power(v[i]);
    } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) seg[i] = add_rn(seg[i], pspec_power(v[i]));
    }
}
// a finished segment into the row accumulator, over the R registers a lane holds (16 here, 17 in the real plan's fused kernel)
template <int R>
RD_HD void pspec_fold_regs(const float (&seg)[R], float (&row)[R], bool first)
{
    if (first) {
#pragma unroll
        for (int i = 0; i < R; ++i) row[i] = seg[i];
    } else {
#pragma unroll
        for (int i = 0; i < R; ++i) row[i] = add_rn(row[i], seg[i]);
    }
}
RD_HD void pspec1k_fold(const float (&seg)[16], float (&row)[16], bool first) { pspec_fold_regs(seg, row, first); }
// dst: the unit's 1024 f32 (a row of the output, or a segment's partial)
template <typename OutPtr>
RD_HD void pspec1k_store(const float (&row)[16], OutPtr dst, int lane)
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j) dst[lane + 64 * q + 256 * j] = row[4 * q + j];
}

// ---- the same kernel fed with the receiver's interleaved u8 I/Q bytes (redio_pspec_enqueue_u8): a sample is one little-endian 16-bit
// word, I in the low byte and Q in the high one (rtlsdr.rs:159-162), so a transform that starts on any sample is 2-byte aligned and
// a wave-wide 16-bit load covers 128 contiguous bytes.  x: 16-bit words.
RD_HD float2 pspec_iq(unsigned word) { return make_float2(i2f(word & 0xffu), i2f((word >> 8) & 0xffu)); }
template <typename BPtr>
RD_HD void pspec1k_load_raw(uint16_t (&r)[16], BPtr x, int lane)
{
#pragma unroll
    for (int t = 0; t < 16; ++t) r[t] = x[lane + 64 * t];
}
RD_HD void pspec1k_convert(float2 (&v)[16], const uint16_t (&r)[16])
{
#pragma unroll
    for (int t = 0; t < 16; ++t) v[t] = pspec_iq(r[t]);
}

// ---- the generic passes' thread programs
// the row gather from bytes: element n of row b = sample b step + n converted, times win[n] when there is a window
template <typename BPtr, typename WPtr>
RD_HD float2 pspec_rows_u8_thread(BPtr x, WPtr win, bool windowed, long b, long n, long step)
{
    float2 v = pspec_iq(x[b * step + n]);
    if (windowed) {
        const float wn = win[n];
        v = make_float2(mul_rn(v.x, wn), mul_rn(v.y, wn));
    }
    return v;
}
// lane step q of the gather: elements 2 q and 2 q + 1 of the packed rows, which share one 16-byte store (the second may open the next row)
template <typename BPtr, typename WPtr>
RD_HD void pspec_rows_u8_pair(BPtr x, WPtr win, bool windowed, unsigned q, unsigned N, long step, float2 &v0, float2 &v1)
{
    const unsigned i = 2 * q, b = i / N, n = i - b * N;
    const bool wraps = n + 1 == N;
    v0 = pspec_rows_u8_thread(x, win, windowed, (long)b, (long)n, step);
    v1 = pspec_rows_u8_thread(x, win, windowed, (long)(wraps ? b + 1 : b), (long)(wraps ? 0 : n + 1), step);
}
// spec: the segment's first spectrum (rows of N bins); returns seg[k]
template <typename SPtr>
RD_HD float pspec_accum_thread(SPtr spec, long N, long cnt, long k)
{
    float a = pspec_power(spec[k]);
    for (long i = 1; i < cnt; ++i) a = add_rn(a, pspec_power(spec[i * N + k]));
    return a;
}
// part: the row's first partial (S partials of N f32); returns out[r][k]
template <typename PPtr>
RD_HD float pspec_fold_thread(PPtr part, long N, long S, long k)
{
    float a = part[k];
    for (long s = 1; s < S; ++s) a = add_rn(a, part[s * N + k]);
    return a;
}

} // namespace redio
