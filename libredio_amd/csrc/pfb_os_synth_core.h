// pfb_os_synth_core.h -- index maps and launch geometry of the oversampled synthesis bank (include/redio_pfb_os_synth.h, redio_pfb_os_synth_*).
//
// The way back from the oversampled channelizer's rows (pfb_os_core.h) to one stream, a weighted overlap-add: per row kissfft's
// unnormalised M-point inverse transform w_r, then output sample n = q H + j at absolute time tau = (F + L - 1) H + n is the strict left
// fold of dsputils::convolve (dsputils.rs:31) over the rows r = q + k, k = k0_j .. L - 1 (L = ceil(P M / H)), of
// w_r[tau mod M] * h[tap(o)], o = (L - 1 - k) H + j the offset of tau in row r's window, tap(o) = (P - 1 - o div M) M + o mod M.
// At H = M this is pfb_synth_core.h's bank term for term.
//
// Route 1 (M = 64, H = 32, P in {4, 8, 16}; L = 2 P) is pfb_synth64_kernel up to exchange 3, after which lane c holds column c of the
// tile's sixteen w_r.  tau mod 64 = j + 32 ((F + q + 1) & 1): lane c = j + 32 b produces an output only for the hops q with
// (F + q + 1) & 1 == b, every other hop, from the 2 P rows q .. q + 2 P - 1 of its own column.  o div 64 = P - 1 - (k >> 1) and
// o mod 64 = j + 32 (1 - (k & 1)), so the tap of step k, h[64 (k >> 1) + j + 32 (1 - (k & 1))], does not depend on b.  Tiles start on
// even rows of the call; rows are walked in pairs (r0, r0 + 1), r0 even.  Row r completes hop r - (2 P - 1), so a pair completes the
// hops q0 = r0 - (2 P - 1) and q0 + 1: the lanes with b == F & 1 ("early") own q0, whose window ends at row r0, the others own q0 + 1,
// whose window ends at r0 + 1.  The early half reads exchange 3's tile one row behind the other half (row -1 of a tile is the last row of
// the tile before, carried in one register), so that both halves fold the same 2 P window registers with the same taps, and the 64
// results of a pair are the 64 consecutive samples from 32 q0 on.
// Host-compilable (tests/emu_pfb_os_synth).
#pragma once
#include "pfb_os_core.h"
#include "pfb_synth_core.h"

namespace redio {

// ---- the contract's index arithmetic (route 0's overlap-add pass, and the emulation) ----
RD_HD long pfboss_L(long M, long P, long H) { return (P * M + H - 1) / H; }
// the first row offset that takes part: the oldest row's window ends before residue j when (L - 1) H + j >= P M
RD_HD long pfboss_k0(long j, long M, long P, long H, long L) { return (L - 1) * H + j >= P * M ? 1 : 0; }
RD_HD long pfboss_offset(long k, long j, long H, long L) { return (L - 1 - k) * H + j; }
RD_HD long pfboss_tap(long o, long M, long P) { return (P - 1 - o / M) * M + o % M; }
// tau mod M for hop q of a pass whose first row has F mod M = f0: ((F + L - 1 + q) H + j) mod M
RD_HD long pfboss_col(long f0, long q, long j, long M, long H, long L) { return ((f0 + (L - 1) % M + q % M) % M * H + j) % M; }

// ---- route 1, launch geometry: launch_pfb_t's decision (pfb_kernels.hip) on output hops ----
// a wavefront owns the hops [t0, t1) = a contiguous run of hops_per_wave (a multiple of the tile, at least 4 tiles) and walks the input
// rows t0 ... t1 + 2 P - 2 in tiles of 16 that start at t0; the first 2 P - 1 rows of a run are its halo
constexpr long PFBOSS_WAVES = 8L * 256;
RD_HD long pfboss_hops_per_wave(long hops)
{
    long hpw = (hops + PFBOSS_WAVES - 1) / PFBOSS_WAVES;
    hpw = ((hpw + PFB_TILE - 1) / PFB_TILE) * PFB_TILE;
    return hpw < 4 * PFB_TILE ? 4 * PFB_TILE : hpw;
}
RD_HD long pfboss_waves(long hops) { const long hpw = pfboss_hops_per_wave(hops); return (hops + hpw - 1) / hpw; }
// input row a tile asks for, clamped by address to the last row of the call (T - 1 = hops + 2 P - 2): a clamped row completes only
// hops at or past the last one
RD_HD long pfboss_in_row(long r, long hops, int P) { const long last = hops + 2 * P - 2; return r < last ? r : last; }

// ---- route 1, the hop-32 overlap-add behind exchange 3 ----
RD_HD int pfboss_early(int lane, int fpar) { return (lane >> 5) == fpar; }
// the tap of fold step k (ascending row) in lane `lane`
RD_HD int pfboss_tap64(int lane, int k) { return PFB_M * (k >> 1) + (lane & 31) + PFBOS_H * (1 - (k & 1)); }
// exchange 3's tile row that enters a lane's window as tile row ti >= 1: row ti - 1 for the early half, ti for the other one, as one
// per-lane base and an offset that is the same in every lane (never negative).  Tile row 0 is the carried row for the early half and
// pfbs_x3_load(0, lane) for the other one
RD_HD int pfboss_x3_base(int lane, int early) { return pfbs_x3_load(1 - early, lane); }
RD_HD int pfboss_x3_load(int base, int ti) { return base + (ti - 1) * PFBS_ROW3; }
// window slots: pair n of a run (n = 8 tile + u) writes slots 2 n and 2 n + 1 mod 2 P; fold step k then reads slot 2 n + 2 + k.  A tile
// moves the window by 16 slots: at P = 16 the odd tiles of a run start at slot 16, at P = 4 and 8 every tile starts at slot 0
RD_HD int pfboss_slot_new(int tile_par, int u, int P) { return (PFB_TILE * tile_par + 2 * u) % (2 * P); }
RD_HD int pfboss_slot(int tile_par, int u, int k, int P) { return (PFB_TILE * tile_par + 2 * u + 2 + k) % (2 * P); }
// the hop q0 the early half completes with the pair that starts at input row r0 (the other half completes q0 + 1), and where a lane's
// sample goes among the 64 from 32 q0 on
RD_HD long pfboss_hop(long r0, int P) { return r0 - (2 * P - 1); }
RD_HD int pfboss_out_pos(int lane, int early) { return (lane & 31) + (early ? 0 : PFBOS_H); }

} // namespace redio
