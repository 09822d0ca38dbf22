"""The polyphase spectrometer restated: oracle.pfb_channelizer's rows through pspec_ref.spectra -- the checker of
redio_pfb_pspec_*.  Nothing is computed here that those two do not compute."""
import numpy as np

import oracle
import pspec_ref


def shape(M, P, K):
    """(W, H) in samples: what one output row needs, and the samples between the starts of two rows"""
    return (K - 1 + P) * M, K * M


def nrows(n, M, P, K):
    T = n // M
    return 0 if T < P + K - 1 else (T - P + 1) // K


def channel_rows(x, h, M, P, K, fused=False):
    """the channelizer's rows that whole output rows integrate"""
    rows = oracle.pfb_channelizer(x, h, M, P, fused)
    return rows[: len(rows) // K * K]


def spectrum(x, h, M, P, K, fused=False):
    rows = channel_rows(x, h, M, P, K, fused)
    return pspec_ref.spectra(rows, M, K) if len(rows) else np.empty((0, M), np.float32)


def spectrum_u8(raw, h, M, P, K, fused=False):
    return spectrum(oracle.data_to_samples(raw), h, M, P, K, fused)
