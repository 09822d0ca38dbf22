"""The oversampled synthesis bank's contract (include/redio_pfb_os_synth.h, redio_pfb_os_synth_*) restated on the oracle: one
oracle.fft(inverse=True) per row, then per output residue j and per phase of the column one oracle.fir.  It adds no arithmetic of its
own.  Also nout, route, the one-kernel route's launch geometry (libredio_amd/csrc/pfb_os_synth_core.h) and a model of the stream
(redio_pfb_os_synth_stream_*)."""
import math

import numpy as np

import oracle
import pfb_synth_ref

TILE = 16      # PFB_TILE: input rows per wave tile
WAVES = 2048   # PFBOSS_WAVES: wavefronts the launcher aims for


def nrows_per_hop(M, P, H):
    """L = ceil(P M / H): the rows that make one hop of output"""
    return -(-(P * M) // H)


def nhops(n_in, M, P, H):
    T = n_in // M
    return max(T - nrows_per_hop(M, P, H) + 1, 0)


def nout(n_in, M, P, H):
    return nhops(n_in, M, P, H) * H


def route(M, P, H):
    """1: the 64-channel wave kernel at hop 32, 0: two passes"""
    return 1 if M == 64 and H == 32 and P in (4, 8, 16) else 0


def hops_per_wave(hops):
    hpw = -(-hops // WAVES)
    hpw = -(-hpw // TILE) * TILE
    return max(hpw, 4 * TILE)


def waves(hops):
    return -(-hops // hops_per_wave(hops))


def tap(o, M, P):
    """the prototype's tap at window offset o"""
    return (P - 1 - o // M) * M + o % M


def k0(j, M, P, H):
    """the first row offset that takes part at residue j: the oldest row drops out where its window offset would pass P M"""
    L = nrows_per_hop(M, P, H)
    return 1 if (L - 1) * H + j >= P * M else 0


def column(F, q, j, M, P, H):
    """tau mod M for output sample q H + j, tau = (F + L - 1 + q) H + j"""
    return ((F + nrows_per_hop(M, P, H) - 1 + q) * H + j) % M


inverse_rows = pfb_synth_ref.inverse_rows  # step 1: kissfft's unnormalised M-point inverse transform of every whole row -> [T][M]


def overlap_add(W, h, M, P, H, F=0, fused=False):
    """step 2 on rows W [T][M]: y[q H + j] = the fold of dsputils::convolve over w_{q+k}[tau mod M] * h[tap((L - 1 - k) H + j)] in
    ascending k = k0_j .. L - 1.  The column tau mod M depends on q only through q mod (M / gcd(M, H)): one oracle.fir per residue j and
    phase on the column W[k0_j:, c], keeping the q of that phase."""
    h = np.ascontiguousarray(h, np.float32)
    assert len(h) == M * P and 1 <= H <= M
    L = nrows_per_hop(M, P, H)
    hops = max(W.shape[0] - L + 1, 0)
    y = np.empty((hops, H), np.complex64)
    period = M // math.gcd(M, H)
    for j in range(H if hops else 0):
        kj = k0(j, M, P, H)
        taps = np.ascontiguousarray(h[[tap((L - 1 - k) * H + j, M, P) for k in range(kj, L)]])
        for ph in range(min(period, hops)):
            c = column(F, ph, j, M, P, H)
            y[ph::period, j] = oracle.fir(np.ascontiguousarray(W[kj:, c]), taps, 1, fused)[ph::period]
    return y.reshape(-1)


def synth(X, h, M, P, H, F=0, fused=False):
    """the whole contract: n_in cf32 values (rows of M channels; a trailing partial row ignored) -> (T - L + 1) H samples of one stream"""
    return overlap_add(inverse_rows(X, M), h, M, P, H, F, fused)


class StreamModel:
    """redio_pfb_os_synth_stream_*: L - 1 whole rows and the values of a partial row carried, and the running row index"""

    def __init__(self, h, M, P, H, fused=False):
        self.h, self.M, self.P, self.H, self.fused = h, M, P, H, fused
        self.reset()

    def reset(self):
        self.tail, self.row = np.empty(0, np.complex64), 0

    @property
    def pending(self):
        return len(self.tail)

    def nout(self, n_new):
        return nout(len(self.tail) + n_new, self.M, self.P, self.H)

    def feed(self, X):
        buf = np.concatenate([self.tail, np.ascontiguousarray(X, np.complex64)])
        out = synth(buf, self.h, self.M, self.P, self.H, self.row, self.fused)
        hops = len(out) // self.H
        self.row += hops
        self.tail = buf[hops * self.M:]
        return out
