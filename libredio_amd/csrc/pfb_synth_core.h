// pfb_synth_core.h -- lane programs, index maps and launch geometry of the 64-channel synthesis filterbank (include/redio.h, redio_pfb_synth_*).
//
// The channelizer is "branch filter, then forward transform".  This is "inverse transform, then the same branch filter": per row
// kissfft's unnormalised 64-point inverse transform (the pfb_core.h lane programs with INV = true), then per branch m the strict left
// fold of dsputils::convolve (dsputils.rs:31) over P taps g_m[p] = h[64 p + m] on the column v_t[m] of transformed rows.
//
// One wavefront works on 16 consecutive INPUT rows, pfb64_kernel's tile run the other way round: the rows arrive lane = channel (one
// 512-byte row per wave instruction), exchange 1 turns them into the transform's layout (lane (tt, d0) holds channels d0 + 4 e of row tt),
// passes A/B | exchange 2 | pass C leave lane (tt, k1) with X[k2 + 4 k1 + 16 k0], and exchange 3 turns the tile back to lane = branch for
// the filters, whose P-row window lives in registers.  Exchanges 1 and 2 are pfb_core.h's own maps; exchange 3 is below.
// Host-compilable (tests/emu_pfb_synth).
#pragma once
#include "pfb_core.h"

namespace redio {

// exchange 3: lane (tt, k1) stores value (k0, k2) = channel k2 + 4 k1 + 16 k0 of row tt; lane = branch m loads row ti.
// Row stride 65 (float2), not PFB_ROW: a store instruction (fixed k0, k2) has the 16 lanes of a ds_write_b64 group at dword
// 130 tt + 8 k1 + const, and 130 = 2 (mod 32) spreads four consecutive tt over the even banks between the 8 k1 steps -- all 32 banks,
// one lane each.  With PFB_ROW = 68 (136 = 8 mod 32) tt and k1 would land on the same four bank pairs, a 4-way conflict: 68 is padded
// for exchange 1 and 2, whose lanes differ in d0 (2 dwords), not in k1 (8).  The loads are 64 consecutive float2, conflict-free at any stride.
constexpr int PFBS_ROW3 = 65;
static_assert(PFB_TILE * PFBS_ROW3 <= PFB_LDS, "exchange 3 fits the wave's tile");
RD_HD int pfbs_x3_store(int lane, int k0, int k2) { return (lane >> 2) * PFBS_ROW3 + pfb_out_channel(lane, k0, k2); }
RD_HD int pfbs_x3_load(int ti, int lane) { return ti * PFBS_ROW3 + lane; }

// ---- launch geometry: launch_pfb_t's decision (pfb_kernels.hip) on OUTPUT rows ----
// a wavefront owns output rows [t0, t1) = a contiguous run of rows_per_wave (a multiple of the tile, at least 4 tiles), and walks input
// rows t0 ... t1 + P - 2 in tiles of 16 that start at t0: input row r completes output row r - P + 1, so the first P - 1 rows of a run
// produce nothing (the run's halo: one extra tile per wave whenever the run is a whole number of tiles)
constexpr long PFBS_WAVES = 8L * 256;
RD_HD long pfbs_rows_per_wave(long rows)
{
    long rpw = (rows + PFBS_WAVES - 1) / PFBS_WAVES;
    rpw = ((rpw + PFB_TILE - 1) / PFB_TILE) * PFB_TILE;
    return rpw < 4 * PFB_TILE ? 4 * PFB_TILE : rpw;
}
RD_HD long pfbs_waves(long rows) { const long rpw = pfbs_rows_per_wave(rows); return (rows + rpw - 1) / rpw; }
// input row a tile asks for, clamped by address to the last row of the stream (T - 1 = rows + P - 2): only rows that complete an
// output at or past t1 are ever clamped
RD_HD long pfbs_in_row(long r, long rows, int P) { const long last = rows + P - 2; return r < last ? r : last; }
// the store predicate of input row r in the run [t0, t1)
RD_HD bool pfbs_stores(long r, long t0, long t1, int P) { const long t = r - (P - 1); return t >= t0 && t < t1; }

} // namespace redio
