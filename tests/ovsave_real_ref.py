"""Overlap-save on a real stream in numpy float32 over tests/fftr_ref.py: the checker of redio_ovsave_real_*.
Every multiply and add is one float32 operation."""
import numpy as np

import fftr_ref

F = np.float32


def shape(ntaps, N):
    """(Ke, hop): an even tap count counts as one more, so that hop is even"""
    assert N >= 2 and N % 2 == 0 and ntaps >= 1 and (ntaps | 1) <= N
    return ntaps | 1, N - (ntaps | 1) + 1


def nout(n, ntaps, N):
    hop = shape(ntaps, N)[1]
    return ((n - N) // hop + 1) * hop if n >= N else 0


def spectrum(taps, N):
    """Hc = conj(kiss_fftr(taps zero-padded to N)) as (real, imag)"""
    hp = np.zeros(N, F)
    hp[: len(taps)] = np.asarray(taps, F)
    H = fftr_ref.fftr(hp)
    return H.real.copy(), -H.imag


def product(X, Hc):
    Y = np.empty(len(X), np.complex64)
    Y.real = X.real * Hc[0] - X.imag * Hc[1]
    Y.imag = X.real * Hc[1] + X.imag * Hc[0]
    return Y


def overlap_save_real(x, taps, N):
    x = np.ascontiguousarray(x, F)
    hop, Hc, scale = shape(len(taps), N)[1], spectrum(taps, N), F(1.0) / F(N)
    out = np.empty(nout(len(x), len(taps), N), F)
    for b in range(len(out) // hop):
        y = fftr_ref.fftri(product(fftr_ref.fftr(x[b * hop: b * hop + N]), Hc))
        out[b * hop: (b + 1) * hop] = y[:hop] * scale
    return out
