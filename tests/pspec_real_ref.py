"""The real-input integrated power spectrum in numpy float32: the checker of redio_pspec_real_*.  The gather and the
window multiply are here; the transform is fftr_ref's kiss_fftr, the squaring and the blocked sum are pspec_ref's."""
import numpy as np

import fftr_ref
import pspec_ref

F = np.float32
SEG = pspec_ref.SEG


def shape(N, K, step):
    """(W, H) in real samples: what one row needs, and the distance between the starts of two rows"""
    assert N >= 2 and N % 2 == 0
    return pspec_ref.shape(N, K, step)


def nrows(n, N, K, step):
    W, H = shape(N, K, step)
    return 0 if n < W else (n - W) // H + 1


def nbins(N):
    return N // 2 + 1


def gather(x, N, K, step=None, window=None):
    """the rows the transforms read: nrows * K rows of N float32, times the window when there is one"""
    x = np.ascontiguousarray(x, F)
    step = N if step is None else step
    nt = nrows(len(x), N, K, step) * K
    rows = np.stack([x[t * step: t * step + N] for t in range(nt)]) if nt else np.empty((0, N), F)
    if window is not None:
        rows = rows * np.asarray(window, F)
    return rows


def power_spectrum(x, N, K, step=None, window=None):
    rows = gather(x, N, K, step, window)
    if not len(rows):
        return np.empty((0, nbins(N)), F)
    return pspec_ref.integrate(pspec_ref.power(fftr_ref.fftr_rows(rows, N)), K)


def spectra(X, N, K):
    """the integration alone over packed, already transformed rows of N / 2 + 1 bins"""
    return pspec_ref.integrate(pspec_ref.power(np.ascontiguousarray(X, np.complex64).reshape(-1, nbins(N))), K)
