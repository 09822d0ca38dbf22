// pfb_pspec_core.h -- lane programs of the fused 64-channel polyphase spectrometer (redio_pfb_pspec_*; contract: DESIGN.md 5.6b)
// behind the channelizer's transform (pfb_core.h): the power tile that turns "lane = 16 bins of one row" into "lane = one channel of
// sixteen rows", and the blocked sum of pspec_core.h as a state machine over consecutive channelizer rows.
//
//     p_t[c]    = row_t[c].re * row_t[c].re + row_t[c].im * row_t[c].im        every multiply and add rounded on its own
//     out[r][c] = the fold of pspec_core.h over t in [r K, r K + K): segments of PSPEC_SEG rows counted from r K
//
// Host-compilable (tests/emu_pfb_pspec runs the same programs on the CPU).
#pragma once
#include "pfb_core.h"
#include "pspec_core.h"

namespace redio {

// The power tile: 16 rows x 64 channels of f32 in the wave's own LDS region (5 KiB of its 8.5), row stride 80.  A lane reads one
// channel of every row (consecutive lanes, consecutive words: conflict-free at any stride); it writes 16-byte runs at word
// 80 tt + 4 k1 + 16 k0, and 80 = 16 mod 32 spreads the (tt, k1) of a wave instruction evenly over the 32 banks a write counts.
constexpr int PFBSPEC_ROW = 80;
constexpr int PFBSPEC_LDS = PFB_TILE * PFBSPEC_ROW; // f32
static_assert(PFBSPEC_LDS * sizeof(float) <= PFB_LDS * sizeof(float2), "the power tile lies inside the wave's exchange region");

// Auto mode (redio_pfb_pspec_set_split(h, 0)) lets a wave own whole output rows when those runs give at least this many waves, and
// runs of whole segments otherwise: the wave count from which the channelizer's kernel measured flat
// (profiles/r04_channelizer_64_experiments.txt).
constexpr long PFBSPEC_SPLIT_WAVES = 1024;

// Consecutive units one wavefront owns: whole units, at least four 16-row tiles of channelizer rows so that the P - 1 row prologue
// is amortised, aiming at the 2048 waves of the channelizer's launch (pfb_kernels.hip, launch_pfb_t)
RD_HD long pfbspec_units_per_wave(long nunits, long K, bool split)
{
    const long waves = 8L * 256;
    const long per_unit = split ? PSPEC_SEG : K; // rows of a unit (a row's last segment may hold fewer)
    const long upw = (nunits + waves - 1) / waves, least = (4 * PFB_TILE + per_unit - 1) / per_unit;
    return upw < least ? least : upw;
}

RD_HD int pfbspec_tile_index(int tt, int ch) { return tt * PFBSPEC_ROW + ch; }

// after pfb_fft64_passC lane (tt, k1) holds w[k0 + 4 k2] = X[k2 + 4 k1 + 16 k0] of row tt: the powers of the four consecutive
// channels 16 k0 + 4 k1 + (0 ... 3), one 16-byte run of the tile at pfbspec_tile_index(tt, pfb_out_channel(lane, k0, 0))
RD_HD float4 pfbspec_power4(const float2 (&w)[16], int k0)
{
    return make_float4(pspec_power(w[k0]), pspec_power(w[k0 + 4]), pspec_power(w[k0 + 8]), pspec_power(w[k0 + 12]));
}

// The fold over consecutive channelizer rows.  A unit is an output row (K channelizer rows) or, with `split`, one segment of
// one (at most PSPEC_SEG).  Everything here is wave-uniform; the two accumulators are the lane's.
struct PfbSpecFold {
    long u;    // the unit being summed
    long i;    // its next row, 0 ... cnt - 1
    long cnt;  // rows it holds
    long left; // split: rows of its output row that lie behind it
};
// t0: the unit's first channelizer row, counted from the call's first
RD_HD void pfbspec_fold_begin(PfbSpecFold &f, long u0, long K, bool split, long &t0)
{
    f.u = u0; f.i = 0; f.left = 0;
    pspec_unit(u0, K, split, t0, f.cnt);
    if (split) {
        const long S = pspec_nseg(K), s = u0 % S;
        f.left = K - (long)PSPEC_SEG * s - f.cnt;
    }
}
// the first row behind unit u1 - 1: a wave that owns units [u0, u1) sums rows [t0, t1)
RD_HD long pfbspec_units_end(long u1, long K, bool split)
{
    long g, cnt;
    pspec_unit(u1 - 1, K, split, g, cnt);
    return g + cnt;
}
// power p of the next row into the accumulators.  With the unit's last row the lane stores dst[64 u + lane] (a row of the
// output, or a segment's partial) and the machine moves to the next unit.
template <typename OutPtr>
RD_HD void pfbspec_fold_step(PfbSpecFold &f, float p, float &seg, float &row, long K, bool split, OutPtr dst, int lane)
{
    const PspecStep s = pspec_step(f.i, f.cnt);
    seg = s.seg_first ? p : add_rn(seg, p);
    if (s.seg_last) row = s.row_first ? seg : add_rn(row, seg);
    if (++f.i == f.cnt) {
        dst[f.u * PFB_M + lane] = row;
        ++f.u; f.i = 0;
        if (split) {
            if (f.left == 0) f.left = K;
            f.cnt = f.left < PSPEC_SEG ? f.left : PSPEC_SEG;
            f.left -= f.cnt;
        }
    }
}

} // namespace redio
