"""The synthesis filterbank's contract (include/redio.h, redio_pfb_synth_*) restated on the oracle: "inverse transform, then the same
branch filter" -- one oracle.fft(inverse=True) per row, one oracle.fir per branch.  It adds no arithmetic of its own.  Also nout, route
and the one-kernel route's launch geometry (libredio_amd/csrc/pfb_synth_core.h)."""
import numpy as np

import oracle

TILE = 16      # PFB_TILE: input rows per wave tile
WAVES = 2048   # PFBS_WAVES: wavefronts the launcher aims for


def nrows(n_in, M, P):
    T = n_in // M
    return max(T - P + 1, 0)


def nout(n_in, M, P):
    return nrows(n_in, M, P) * M


def route(M, P):
    """1: the 64-channel wave kernel, 0: two passes"""
    return 1 if M == 64 and P in (4, 8, 16) else 0


def rows_per_wave(rows):
    rpw = -(-rows // WAVES)
    rpw = -(-rpw // TILE) * TILE
    return max(rpw, 4 * TILE)


def waves(rows):
    return -(-rows // rows_per_wave(rows))


def inverse_rows(X, M):
    """step 1: kissfft's unnormalised M-point inverse transform of every whole row -> [T][M]"""
    X = np.ascontiguousarray(X, np.complex64).reshape(-1)
    T = len(X) // M
    if T == 0:
        return np.empty((0, M), np.complex64)
    return oracle.fft(X[: T * M], M, inverse=True).reshape(T, M)


def filter_rows(V, h, M, P, fused=False):
    """step 2 on rows V [T][M]: per branch m the fold of dsputils::convolve over v_{t+p}[m] * h[M p + m] -> [T - P + 1][M]"""
    h = np.ascontiguousarray(h, np.float32)
    assert len(h) == M * P
    T = V.shape[0]
    rows = max(T - P + 1, 0)
    out = np.empty((rows, M), np.complex64)
    if rows:
        for m in range(M):
            out[:, m] = oracle.fir(np.ascontiguousarray(V[:, m]), h[m::M], 1, fused)
    return out


def synth(X, h, M, P, fused=False):
    """the whole contract: n_in cf32 values (rows of M channels; a trailing partial row ignored) -> (T - P + 1) M samples of one stream"""
    return filter_rows(inverse_rows(X, M), h, M, P, fused).reshape(-1)
