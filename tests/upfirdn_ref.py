"""What the rational resampler (redio_upfirdn_*) must give, from the oracle's FIR alone: phase r of the contract (include/redio.h) is the
decimating FIR of dsputils::convolve (dsputils.rs:30-32) with the sub-filter taps[j0 + U t], begun s(r) samples in.  Nothing is computed
here.  Also the route, the tile geometry of DESIGN.md 5.2c and the zero-stuffed form the plan replaces."""
import math

import numpy as np

import oracle

TILED_D = (1, 2, 3, 4, 5, 8, 10)
LDS_WANT, LDS_MAX, TILED_MAX_PERIOD_OUT = 52 * 1024, 150 * 1024, 16


def periods(U, D):
    g = math.gcd(U, D)
    return U // g, D // g


def phases(K, U, D):
    """[(j0, s, K(r))] for r in [0, U')"""
    out = []
    for r in range(periods(U, D)[0]):
        j0 = (-(r * D)) % U
        out.append((j0, (r * D + j0) // U, -(-(K - j0) // U) if K > j0 else 0))
    return out


def window(K, U, D):
    return ((periods(U, D)[0] - 1) * D + K - 1) // U + 1


def nout(n, K, U, D):
    return 0 if n * U < K else (n * U - K) // D + 1


def lds_elems(R, K, U, D):
    Up, Dp = periods(U, D)
    t, lstr = (256 * R - 1) * Dp + window(K, U, D), R * Dp
    return (t + (t // lstr if lstr % 2 == 0 else 0) + 4) // 4 * 4 + 256 * R * Up


def periods_per_lane(K, U, D):
    """R of route 1: the largest of 4, 2, 1 (D' of 8 and 10: of 2, 1) whose tile (as cf32) fits 52 KiB, else the largest that fits
    150 KiB, else 0"""
    for limit in (LDS_WANT, LDS_MAX):
        for R in ((4, 2, 1) if periods(U, D)[1] < 8 else (2, 1)):
            if lds_elems(R, K, U, D) * 8 <= limit:
                return R
    return 0


def route(K, U, D):
    Up, Dp = periods(U, D)
    return 1 if Dp in TILED_D and Up <= TILED_MAX_PERIOD_OUT and K <= 2 ** 20 and periods_per_lane(K, U, D) else 2


def lane_pass(K, U, D):
    """(R, pass) of periods_per_lane: pass 1 inside LDS_WANT, pass 2 inside LDS_MAX; (0, 0) where no tile fits"""
    for pas, limit in ((1, LDS_WANT), (2, LDS_MAX)):
        for R in ((4, 2, 1) if periods(U, D)[1] < 8 else (2, 1)):
            if lds_elems(R, K, U, D) * 8 <= limit:
                return R, pas
    return 0, 0


def regimes(U, D, kmax=2 ** 20):
    """[(first K, R, pass, route)] over K in [1, kmax]: a new row wherever (R, pass, route) changes.  lds_elems never falls as K grows,
    so each (R, limit) fits up to one K found by bisection, and nothing changes between those."""
    edges = {1}
    for limit in (LDS_WANT, LDS_MAX):
        for R in (4, 2, 1):
            if lds_elems(R, 1, U, D) * 8 > limit:
                continue
            lo, hi = 1, kmax
            while lo < hi:
                mid = (lo + hi + 1) // 2
                lo, hi = (mid, hi) if lds_elems(R, mid, U, D) * 8 <= limit else (lo, mid - 1)
            if lo < kmax:
                edges.add(lo + 1)
    rows = []
    for K in sorted(edges):
        row = lane_pass(K, U, D) + (route(K, U, D),)
        if not rows or rows[-1][1:] != row:
            rows.append((K,) + row)
    return rows


def tile_out(K, U, D):
    """outputs one workgroup produces: 256 lanes x R periods x U' on route 1, 256 on route 2"""
    return 256 * periods_per_lane(K, U, D) * periods(U, D)[0] if route(K, U, D) == 1 else 256


def n_for(n_out, K, U, D):
    """the shortest input that yields n_out outputs (n_out >= 1)"""
    return -(-((n_out - 1) * D + K) // U)


def upfirdn(x, taps, U, D, fused=False, count=None):
    """the first `count` outputs (default: all nout) of the contract, every phase one oracle.fir call"""
    x, taps = np.asarray(x), np.asarray(taps, np.float32)
    K = len(taps)
    Up, Dp = periods(U, D)
    total = nout(len(x), K, U, D) if count is None else count
    y = np.zeros(total, x.dtype)  # +0 where a phase has no taps
    for r, (j0, s, k) in enumerate(phases(K, U, D)):
        cnt = (total - r + Up - 1) // Up if total > r else 0
        if cnt and k:
            got = oracle.fir(x[s: s + (cnt - 1) * Dp + k], taps[j0::U][:k], Dp, fused)
            assert len(got) == cnt
            y[r::Up] = got
    return y


def zero_stuffed(x, U):
    z = np.zeros(len(x) * U, np.asarray(x).dtype)
    z[::U] = x
    return z


def upfirdn_zero_stuffed(x, taps, U, D, fused=False):
    """the composition the plan replaces: U - 1 zeros behind every sample, then the decimating FIR"""
    return oracle.fir(zero_stuffed(x, U), taps, D, fused)
