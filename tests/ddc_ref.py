"""What the tuner (redio_ddc_*) must give, from the oracle's own blocks alone: kpn::mul_vecs (kpn.rs:198-203) by the oscillator table
tiled from `first`, then the FIR of dsputils::convolve (dsputils.rs:30-32).  Nothing is computed here."""
import math

import numpy as np

import oracle

MAX_PERIOD = 65536


CHUNKED_R = {1: 8, 2: 4, 3: 4, 4: 4, 5: 4, 8: 2, 10: 2}  # outputs per lane of the chunked route (ddc_chunked_r)
CHUNKED_LDS_MAX = 150 * 1024                              # bytes: beyond it the direct kernel runs
TABLE_EXT = 20480                                         # entries behind the period in the device table (DDC_TABLE_EXT)


def chw(decim):
    """whole-chunk size of the chunked route (ddc_chunked_chw)"""
    return 24 if decim == 3 else 40 if decim in (5, 10) else 16


def tile_in(ntaps, decim):
    """samples one workgroup of the chunked route stages (ddc_chunked_tile_in)"""
    return (256 * CHUNKED_R[decim] - 1) * decim + (ntaps + 15) // 16 * 16


def lds_elems(ntaps, decim):
    """cf32 elements of its LDS: the tile, the tail of the last 16-byte load, the pad, the output transpose (ddc_chunked_lds_elems)"""
    r = CHUNKED_R[decim]
    t, lstr = tile_in(ntaps, decim) + 4, r * decim
    return max(t + (t // lstr if lstr % 2 == 0 else 0) + 2, 256 * (r + 1))


def route(ntaps, decim):
    if ntaps in (127, 63) and decim in (1, 5):
        return 1
    return 2 if decim in CHUNKED_R and ntaps <= 2 ** 20 and lds_elems(ntaps, decim) * 8 <= CHUNKED_LDS_MAX else 3


def tile_out(ntaps, decim):
    """outputs one workgroup produces on the route of (ntaps, decim): 256 lanes x outputs per lane"""
    r = route(ntaps, decim)
    if r == 1:
        return 256 * (8 if decim == 1 else 4)
    return 256 * CHUNKED_R[decim] if r == 2 else 256


def last_chunked(decim):
    """the largest tap count the chunked route takes at this decimation (lds_elems never falls as the taps grow)"""
    lo, hi = 1, 2 ** 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if lds_elems(mid, decim) * 8 <= CHUNKED_LDS_MAX else (lo, mid - 1)
    return lo


def tiled(w, first, n):
    w = np.ascontiguousarray(w, np.complex64)
    idx = [(first + i) % len(w) for i in range(n)] if first + n >= 2 ** 63 else (np.arange(n, dtype=np.uint64) + np.uint64(first)) % np.uint64(len(w))
    return w[np.asarray(idx, dtype=np.int64)]


def mixed(x, w, first=0):
    return oracle.zip_vecs(x, tiled(w, first, len(x)))


def ddc(x, w, taps, decim=1, fused=False, first=0):
    return oracle.fir(mixed(x, w, first), taps, decim, fused)


def ddc_u8(raw, w, taps, decim=1, fused=False, first=0):
    return ddc(oracle.data_to_samples(raw), w, taps, decim, fused, first)


def osc_table_ref(num, den):
    """the rule of redio_osc_table with Python's integers and math.cos / math.sin on the same expression"""
    period = den // math.gcd(abs(num), den)
    out = np.empty(period, np.complex64)
    quarter = (1 + 0j, 0 + 1j, -1 + 0j, 0 - 1j)
    for n in range(period):
        k = (num * n) % den
        if (4 * k) % den == 0:
            out[n] = quarter[4 * k // den]
        else:
            a = ((2.0 * math.pi) * float(k)) / float(den)
            out[n] = np.complex64(complex(np.float32(math.cos(a)), np.float32(math.sin(a))))
    return out
