// pfb_os_core.h -- lane programs, index maps and launch geometry of the oversampled polyphase channelizer (include/redio.h, redio_pfb_os_*).
//
// The channelizer with a hop H <= M between rows: row r filters the M P samples from r H on with the channelizer's own branches
// (g_m[p] = h[M p + m], the strict left fold of dsputils::convolve, dsputils.rs:31), turns the M branch sums round by
// s_r = ((F + r) H) mod M places (a permutation: channel k of every row is then referred to absolute time) and takes kissfft's forward
// M-point transform.  At H = M the shift is 0 and this is pfb_core.h's channelizer.
//
// Route 1 (M = 64, H = 32, P in {4, 8, 16}) is pfb64_kernel's tile with a second window.  Lane m of row r needs x[32 (r + 2 p) + m]:
// with the stream cut into HALF-ROWS, s_q[m] = x[32 q + m] for m = 0 .. 63 (512 contiguous bytes, consecutive q overlapping by half),
// row r reads s_r, s_{r+2}, ... s_{r+2(P-1)}.  Rows of one parity share a P-deep window that moves by one half-row of that parity per
// row, so a lane keeps two interleaved windows, even q and odd q, loads every s_q once and rotates both in place.  The shift is 0 or 32:
// it goes into the lane index of exchange 1's store and costs nothing.  Everything behind exchange 1 is pfb_core.h's.
// Host-compilable (tests/emu_pfb_os).
#pragma once
#include "pfb_core.h"

namespace redio {

constexpr int PFBOS_H = 32; // route 1's hop: half a row

// ---- route 1, launch geometry: launch_pfb_t's decision (pfb_kernels.hip) ----
// a wavefront owns output rows [t0, t1) = a contiguous run of rows_per_wave (a multiple of the tile, at least 4 tiles), so every run
// starts on an even row of the call and the parity of F + r inside a tile is that of F + ti
constexpr long PFBOS_WAVES = 8L * 256;
RD_HD long pfbos_rows_per_wave(long rows)
{
    long rpw = (rows + PFBOS_WAVES - 1) / PFBOS_WAVES;
    rpw = ((rpw + PFB_TILE - 1) / PFB_TILE) * PFB_TILE;
    return rpw < 4 * PFB_TILE ? 4 * PFB_TILE : rpw;
}
RD_HD long pfbos_waves(long rows) { const long rpw = pfbos_rows_per_wave(rows); return (rows + rpw - 1) / rpw; }

// half-row a tile asks for, clamped by address to the last one of the stream: row rows - 1 reads up to q = rows - 1 + 2 (P - 1), whose
// last sample 32 q + 63 = 32 (rows - 1) + 64 P - 1 is the last one the call may read
RD_HD long pfbos_half(long q, long rows, int P) { const long last = rows + 2 * P - 3; return q < last ? q : last; }
// sample index of lane `lane` of half-row q
RD_HD long pfbos_in_index(long q, int lane) { return PFBOS_H * q + lane; }
// the half-row that ENTERS the window with row r (tap P - 1), and the window slot of tap p for the j-th row of a parity since the run's start
RD_HD long pfbos_enter(long r, int P) { return r + 2 * (P - 1); }
RD_HD int pfbos_slot(int j, int p, int P) { return (j + p) % P; }
// exchange 1: branch `lane` of tile row ti (tiles start on even rows of the call) goes to v[(lane + s_r) mod 64], s_r = 32 ((F + r) & 1)
RD_HD int pfbos_x1_lane(int lane, int ti, int fpar) { return (lane + PFBOS_H * ((ti + fpar) & 1)) & (PFB_M - 1); }

// ---- route 0: the branch pass with a row stride of H and a rotated store ----
// s_r for row r of a pass whose first row has F mod M = f0: (((F + r) mod M) H) mod M
RD_HD long pfbos_shift(long f0, long r, long M, long H) { return ((f0 + r % M) % M) * H % M; }
RD_HD long pfbos_rot(long m, long s, long M) { const long k = m + s; return k < M ? k : k - M; }

} // namespace redio
