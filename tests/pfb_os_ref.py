"""The oversampled channelizer's contract (include/redio.h, redio_pfb_os_*) restated on the oracle: oracle.fir for the branch sums,
np.roll for the shift, oracle.fft for the rows.  It adds no arithmetic of its own.  Also nrows, route, the one-kernel route's launch
geometry (libredio_amd/csrc/pfb_os_core.h) and a model of the stream (redio_pfb_os_stream_*)."""
import math

import numpy as np

import oracle

TILE = 16      # PFB_TILE: rows per wave tile
WAVES = 2048   # PFBOS_WAVES: wavefronts the launcher aims for


def nrows(n_in, M, P, H):
    return (n_in - M * P) // H + 1 if n_in >= M * P else 0


def route(M, P, H):
    """1: the 64-channel wave kernel at hop 32, 0: two passes"""
    return 1 if M == 64 and H == 32 and P in (4, 8, 16) else 0


def rows_per_wave(rows):
    rpw = -(-rows // WAVES)
    rpw = -(-rpw // TILE) * TILE
    return max(rpw, 4 * TILE)


def waves(rows):
    return -(-rows // rows_per_wave(rows))


def shift(F, r, M, H):
    """s_r = ((F + r) H) mod M"""
    return ((F + r) % M) * H % M


def branch_sums(x, h, M, P, H, fused=False):
    """u_r[m] = the fold of dsputils::convolve over x[r H + M p + m] * h[M p + m] -> [rows][M].  Rows whose r H has the same residue rho
    mod M read whole columns x[rho + m :: M] of the stream: one oracle.fir per branch and residue, out[k] for r H = rho + M k."""
    x = np.ascontiguousarray(x, np.complex64).reshape(-1)
    h = np.ascontiguousarray(h, np.float32)
    assert len(h) == M * P and 1 <= H <= M
    rows = nrows(len(x), M, P, H)
    u = np.empty((rows, M), np.complex64)
    period = M // math.gcd(M, H)
    for r0 in range(min(period, rows)):
        rr = np.arange(r0, rows, period)        # the rows of one residue
        rho = (r0 * H) % M
        k = (rr * H - rho) // M
        for m in range(M):
            col = np.ascontiguousarray(x[rho + m:: M][: k[-1] + P])
            u[rr, m] = oracle.fir(col, h[m::M], 1, fused)[k]
    return u


def rotated(x, h, M, P, H, F=0, fused=False):
    """v_r[(m + s_r) mod M] = u_r[m]: what the transform takes -> [rows][M]"""
    return roll_rows(branch_sums(x, h, M, P, H, fused), M, H, F)


def roll_rows(u, M, H, F):
    """np.roll of every row r of u [rows][M] by s_r, which has a period of M / gcd(M, H) rows: rows r0, r0 + M, ... in one call"""
    v = np.empty_like(u)
    for r0 in range(min(M, u.shape[0])):
        v[r0::M] = np.roll(u[r0::M], shift(F, r0, M, H), axis=1)
    return v


def channelize(x, h, M, P, H, F=0, fused=False):
    """the whole contract: n_in cf32 samples -> [rows][M] cf32, natural channel order"""
    v = rotated(x, h, M, P, H, F, fused)
    if v.shape[0] == 0:
        return v
    return oracle.fft(np.ascontiguousarray(v.reshape(-1)), M, inverse=False).reshape(-1, M)


class StreamModel:
    """redio_pfb_os_stream_*: the unconsumed samples (everything from the next row's first sample on) and the running row index"""

    def __init__(self, h, M, P, H, fused=False):
        self.h, self.M, self.P, self.H, self.fused = h, M, P, H, fused
        self.reset()

    def reset(self):
        self.tail, self.row = np.empty(0, np.complex64), 0

    @property
    def pending(self):
        return len(self.tail)

    def nout(self, n_new):
        return nrows(len(self.tail) + n_new, self.M, self.P, self.H) * self.M

    def feed(self, x):
        buf = np.concatenate([self.tail, np.ascontiguousarray(x, np.complex64)])
        out = channelize(buf, self.h, self.M, self.P, self.H, self.row, self.fused)
        self.row += out.shape[0]
        self.tail = buf[out.shape[0] * self.H:]
        return out.reshape(-1)
