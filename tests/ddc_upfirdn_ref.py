"""What the tuned resampler (redio_ddc_upfirdn_*) must give, from the oracle's own blocks alone: kpn::mul_vecs (kpn.rs:198-203) by the
oscillator table tiled from `first` (tests/ddc_ref.py), then the rational resampler's per-phase reference (tests/upfirdn_ref.py: one
oracle.fir call of dsputils::convolve, dsputils.rs:30-32, per phase).  Nothing is computed here.  The route and the tile size are the
resampler's, on the cf32 geometry."""
import oracle

import ddc_ref
import upfirdn_ref

TABLE_EXT = ddc_ref.TABLE_EXT
route, tile_out, periods, window, nout, n_for = (upfirdn_ref.route, upfirdn_ref.tile_out, upfirdn_ref.periods, upfirdn_ref.window,
                                                 upfirdn_ref.nout, upfirdn_ref.n_for)


def tile_in(K, U, D):
    """samples one workgroup of route 1 stages: (256 R - 1) D' + Wp"""
    Up, Dp = periods(U, D)
    return (256 * upfirdn_ref.periods_per_lane(K, U, D) - 1) * Dp + window(K, U, D)


def ddc_upfirdn(x, w, taps, U, D, fused=False, first=0, count=None):
    return upfirdn_ref.upfirdn(ddc_ref.mixed(x, w, first), taps, U, D, fused, count)


def ddc_upfirdn_u8(raw, w, taps, U, D, fused=False, first=0, count=None):
    return ddc_upfirdn(oracle.data_to_samples(raw), w, taps, U, D, fused, first, count)
