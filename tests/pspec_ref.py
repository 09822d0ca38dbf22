"""The integrated power spectrum in numpy float32 over oracle.fft: the checker of redio_pspec_*.
Every multiply and add is one float32 operation; the sum is blocked in segments of SEG transforms."""
import numpy as np

import oracle

F = np.float32
SEG = 16  # REDIO_PSPEC_SEG


def shape(N, K, step):
    """(W, H): the samples one row needs, and the samples between the starts of two rows"""
    assert N >= 1 and K >= 1 and step >= 1
    return (K - 1) * step + N, K * step


def nrows(n, N, K, step):
    W, H = shape(N, K, step)
    return 0 if n < W else (n - W) // H + 1


def power(X):
    return X.real * X.real + X.imag * X.imag


def integrate(P, K):
    """P: rows of |X|^2, K per output row -> the blocked sum"""
    P = P[: len(P) // K * K].reshape(-1, K, P.shape[-1])
    out = np.empty((P.shape[0], P.shape[2]), F)
    for r in range(P.shape[0]):
        row = None
        for s in range(0, K, SEG):
            seg = P[r, s].copy()
            for t in range(s + 1, min(s + SEG, K)):
                seg = seg + P[r, t]
            row = seg if row is None else row + seg
        out[r] = row
    return out


def power_spectrum(x, N, K, step=None, window=None):
    x = np.ascontiguousarray(x, np.complex64)
    step = N if step is None else step
    nt = nrows(len(x), N, K, step) * K
    rows = np.stack([x[t * step: t * step + N] for t in range(nt)]) if nt else np.empty((0, N), np.complex64)
    if window is not None:
        w = np.asarray(window, F)
        xw = np.empty_like(rows)
        xw.real, xw.imag = rows.real * w, rows.imag * w
        rows = xw
    return integrate(power(oracle.fft(rows.reshape(-1), N).reshape(-1, N)), K) if nt else np.empty((0, N), F)


def spectra(X, N, K):
    """the integration alone over packed, already transformed rows"""
    return integrate(power(np.ascontiguousarray(X, np.complex64).reshape(-1, N)), K)
