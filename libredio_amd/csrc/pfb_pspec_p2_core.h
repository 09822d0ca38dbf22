// pfb_pspec_p2_core.h -- the workgroup form of the polyphase spectrometer (redio_pfb_pspec_*, route 2; contract: DESIGN.md 5.6b)
// for the channel counts of pfb_p2_kernel (32, 128, 256, 512, 1024): the geometry of its row streams and the fold of
// pfb_pspec_core.h for a thread that owns C channels of any row length.
//
// A STREAM is a (thread group, run of consecutive channelizer rows) of pfb_p2_kernel: here it owns whole units [u0, u1) -- output
// rows, or with `split` segments (pspec_unit) -- and sums the channelizer rows [t0, t1) they cover.  G streams share a workgroup,
// which runs max over its streams of ceil((t1 - t0) / TR) iterations of TR rows per stream.
//
// Host-compilable (tests/emu_pfb_pspec_p2 runs the same arithmetic on the CPU).
#pragma once
#include "pfb_pspec_core.h"

namespace redio {

// streams per workgroup and rows per stream and iteration: pfb_p2_kernel's, which for the forms the launcher chooses (one channel per
// thread up to 256 channels; above, M / 256 channels per thread in the 8-byte and in the pair form alike) depend on M alone
RD_HD int pfbspec_p2_streams_per_group(int M) { return M >= 256 ? 1 : 256 / M; }
RD_HD int pfbspec_p2_rows_per_iter(int M) { return M <= 256 ? 16 : 4096 / M; }

// the channelizer's floor: a stream sums at least this many rows, so that its P - 1 row prologue is amortised
constexpr long PFBSPEC_P2_MIN_ROWS = 64;

// Consecutive units one stream owns: whole units, aiming at 4 * cus * G streams (the channelizer's launch), at least the unit count
// that covers PFBSPEC_P2_MIN_ROWS rows of full units (K rows, or with `split` PSPEC_SEG: a row's last segment may hold fewer)
RD_HD long pfbspec_p2_units_per_stream(long nunits, long K, bool split, long cus, int M)
{
    const long streams = 4 * cus * pfbspec_p2_streams_per_group(M);
    const long per_unit = split ? PSPEC_SEG : K;
    const long ups = (nunits + streams - 1) / streams, least = (PFBSPEC_P2_MIN_ROWS + per_unit - 1) / per_unit;
    return ups < least ? least : ups;
}

// Auto mode (redio_pfb_pspec_set_split(h, 0)) lets a stream own whole output rows when those runs fill at least this many workgroups
// per CU, and runs of whole segments otherwise.  Set from a measurement (2^28 samples, K = 32 ... 4096 in both modes
// at 256 x 8 and 1024 x 4 on 256 CUs): by rows is ahead by 1-7 % from 511 workgroups up and behind by 1.4-1.5 x at 255, 2.7 x at 127
// and 5.2 x at 63.  The first guess was 1, the analogue of PFBSPEC_SPLIT_WAVES (1024 waves are one four-wave workgroup per CU).
constexpr long PFBSPEC_P2_SPLIT_GROUPS_PER_CU = 2;
// the row count from which auto mode is rows mode: that many workgroups per CU, G streams each, of the floor's length
RD_HD long pfbspec_p2_split_rows(long K, long cus, int M)
{
    return PFBSPEC_P2_SPLIT_GROUPS_PER_CU * cus * pfbspec_p2_streams_per_group(M) * pfbspec_p2_units_per_stream(1, K, false, cus, M);
}

struct PfbSpecP2Stream {
    long u0, u1; // its units; u0 == u1: a stream behind the last unit, which sums nothing (it still runs the workgroup's barriers)
    long t0, t1; // the channelizer rows they cover, counted from the call's first
};
// stream s of a launch over nunits units that hold `rows` channelizer rows in all
RD_HD PfbSpecP2Stream pfbspec_p2_stream(long s, long ups, long nunits, long rows, long K, bool split)
{
    PfbSpecP2Stream st;
    st.u0 = s * ups;
    if (st.u0 >= nunits) {
        st.u0 = st.u1 = nunits; st.t0 = st.t1 = rows;
        return st;
    }
    st.u1 = st.u0 + ups < nunits ? st.u0 + ups : nunits;
    long cnt;
    pspec_unit(st.u0, K, split, st.t0, cnt);
    st.t1 = pfbspec_units_end(st.u1, K, split);
    return st;
}
RD_HD long pfbspec_p2_stream_iters(const PfbSpecP2Stream &st, int TR) { return (st.t1 - st.t0 + TR - 1) / TR; }

// ---- the fold of pfb_pspec_core.h (PfbSpecFold, pfbspec_fold_begin) for a thread that owns C channels: the counters step once per
// channelizer row, the accumulators once per row and channel.
// power p of one channel of the unit's next row, s = pspec_step(f.i, f.cnt), into that channel's accumulators
RD_HD void pfbspec_p2_fold_accum(const PspecStep &s, float p, float &seg, float &row)
{
    seg = s.seg_first ? p : add_rn(seg, p);
    if (s.seg_last) row = s.row_first ? seg : add_rn(row, seg);
}
// whether that row ends the unit: the row accumulators are then what dst[f.u * M + channel] gets
RD_HD bool pfbspec_p2_fold_ends(const PfbSpecFold &f) { return f.i + 1 == f.cnt; }
// behind every row: the counters move on, into the next unit behind a unit's last row (pfbspec_fold_step's transitions)
RD_HD void pfbspec_p2_fold_next(PfbSpecFold &f, long K, bool split)
{
    if (++f.i == f.cnt) {
        ++f.u; f.i = 0;
        if (split) {
            if (f.left == 0) f.left = K;
            f.cnt = f.left < PSPEC_SEG ? f.left : PSPEC_SEG;
            f.left -= f.cnt;
        }
    }
}

} // namespace redio
