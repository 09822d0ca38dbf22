// pfb_os_p2_core.h -- the workgroup form of the oversampled channelizer (include/redio.h, redio_pfb_os_*, route 2; contract: DESIGN.md
// 5.6d) for the channel counts of pfb_p2_kernel (32, 128, 256, 512, 1024) at a hop of half a row: the geometry of its row streams, the
// half-row a load asks for, the two register windows and the image position of a branch sum.
//
// The stream is cut into overlapping HALF-ROWS s_q[m] = x[(M / 2) q + m], m = 0 .. M - 1 (pfb_os_core.h at 64 channels).  Row r reads
// s_r, s_{r+2}, ... s_{r+2(P-1)}; rows of one parity share a window that moves by one half-row of that parity per row.  A STREAM is a
// (thread group, run of rps consecutive rows) of pfb_p2_kernel; rps is a multiple of the iteration's rows, which are even, so a stream
// starts on an even row of the call and the parity of row tb + ti of an iteration is that of ti.  Per channel a thread keeps, per
// parity, the P - 1 half-rows behind the iteration's first row of that parity (`hist`), and the TR half-rows that enter with the
// iteration's rows (`cur`, in row order): the window of a parity is [hist | cur of that parity].
//
// Host-compilable (tests/emu_pfb_os_p2 runs the same functions on the CPU).
#pragma once
#include "redio_device.h"

namespace redio {

// streams per workgroup and rows per stream and iteration: pfb_p2_kernel's, which for the forms the launcher chooses (one channel per
// thread up to 256 channels; above, M / 256 channels per thread in the 8-byte and in the pair form alike) depend on M alone
RD_HD int pfbos_p2_streams_per_group(int M) { return M >= 256 ? 1 : 256 / M; }
RD_HD int pfbos_p2_rows_per_iter(int M) { return M <= 256 ? 16 : 4096 / M; }

// the channelizer's floor: a stream holds at least this many rows, so that its 2 (P - 1) half-row prologue is amortised
constexpr long PFBOS_P2_MIN_ROWS = 64;

// rows per stream: launch_pfb_p2_t's decision -- about four workgroups per CU, a multiple of the iteration's rows, at least the floor
RD_HD long pfbos_p2_rows_per_stream(long rows, long cus, int M)
{
    const long streams = 4 * cus * pfbos_p2_streams_per_group(M), TR = pfbos_p2_rows_per_iter(M);
    long rps = (rows + streams - 1) / streams;
    rps = ((rps + TR - 1) / TR) * TR;
    return rps < PFBOS_P2_MIN_ROWS ? PFBOS_P2_MIN_ROWS : rps;
}
RD_HD long pfbos_p2_streams(long rows, long rps) { return (rows + rps - 1) / rps; }
RD_HD long pfbos_p2_groups(long rows, long rps, int M)
{
    const long G = pfbos_p2_streams_per_group(M);
    return (pfbos_p2_streams(rows, rps) + G - 1) / G;
}
// rows [t0, t1) of stream s; t0 >= rows: a stream behind the last row, which stores nothing (it still runs the workgroup's barriers)
RD_HD long pfbos_p2_stream_begin(long s, long rps) { return s * rps; }
RD_HD long pfbos_p2_stream_end(long s, long rps, long rows) { const long e = s * rps + rps; return e < rows ? e : rows; }
// iterations of a workgroup: those of its first stream, which holds the most rows
RD_HD long pfbos_p2_group_iters(long group, long rps, long rows, int M)
{
    const long s0 = group * pfbos_p2_streams_per_group(M), TR = pfbos_p2_rows_per_iter(M);
    return (pfbos_p2_stream_end(s0, rps, rows) - pfbos_p2_stream_begin(s0, rps) + TR - 1) / TR;
}

// half-row a load asks for, clamped by address to the last one the call may read: row rows - 1 reads up to q = rows - 1 + 2 (P - 1),
// whose last sample (M / 2) q + M - 1 = (M / 2) (rows - 1) + M P - 1 is the last one of the call's input (pfbos_half)
RD_HD long pfbos_p2_half(long q, long rows, int P) { const long last = rows + 2 * P - 3; return q < last ? q : last; }
// sample index of channel `chan` of half-row q
RD_HD long pfbos_p2_in_index(long q, int chan, int M) { return (long)(M / 2) * q + chan; }
// the half-row in prologue slot p (0 .. P - 2) of parity par of a stream whose first row is t0, and the one that enters with row r
RD_HD long pfbos_p2_hist_half(long t0, int par, int p) { return t0 + par + 2 * p; }
RD_HD long pfbos_p2_enter(long r, int P) { return r + 2 * (P - 1); }
// tap p of local row ti reads element k = (ti >> 1) + p of its parity's window [hist | cur]: hist[k] for k < P - 1, else
// cur[pfbos_p2_cur_slot(ti & 1, k, P)] (cur is in row order: the half-row that entered with local row 2 (k - (P - 1)) + par)
RD_HD int pfbos_p2_win(int ti, int p) { return (ti >> 1) + p; }
RD_HD int pfbos_p2_cur_slot(int par, int k, int P) { return 2 * (k - (P - 1)) + par; }

// leaf position of input index n in the M-point image of fft_p2.h (FftP2<LOG2M>::leaf_pos): the top bit is the radix-2 digit, the
// base-4 digits reverse onto M / 4, M / 16, ...
template <int LOG2M>
RD_HD int pfbos_p2_leaf(int n)
{
    constexpr int L4 = LOG2M / 2, M = 1 << LOG2M;
    int pos = (LOG2M & 1) ? n >> (2 * L4) : 0;
#pragma unroll
    for (int i = 0; i < L4; ++i) pos += ((n >> (2 * i)) & 3) * (M >> (2 * i + 2));
    return pos;
}
// where the branch sum of channel `chan` goes in its row of the image: v_r[(chan + s_r) mod M] with s_r = ((F + r) M / 2) mod M, which is
// M / 2 for odd F + r; r = t0 + TR it + ti with t0 + TR it even, so the parity is that of fpar + ti (fpar = F & 1)
template <int LOG2M>
RD_HD int pfbos_p2_image_pos(int chan, int ti, int fpar)
{
    constexpr int M = 1 << LOG2M;
    return pfbos_p2_leaf<LOG2M>((chan + (M / 2) * ((ti + fpar) & 1)) & (M - 1));
}

} // namespace redio
