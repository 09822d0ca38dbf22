"""An amplitude ladder for the power stage of the spectrum plans (redio_pfb_pspec_*, redio_pspec_*, redio_pspec_real_*).

The special-value inputs of the other tests saturate once squared: their outputs are inf or NaN, never subnormal or zero.  Here the
hash stream is cut into consecutive blocks of 2 H samples (H: the samples between two output rows) and block b is multiplied, in
float32, by rung b: amplitudes whose squares underflow to zero, land among the subnormals, stay normal, or overflow -- in the square,
or only in the sum of finite powers -- and both zeros.  Every class of float32 then turns up in the outputs of one call
(tests/test_spectrum_range_cpu.py holds the restatements to that), so a power stage or a fold that flushes subnormals, or that sums
in a wider type and overflows elsewhere, differs from the restatement (tests/test_gpu_spectrum_range.py).  No input is inf or NaN, and
no output is NaN."""
import numpy as np

import pfb_pspec_ref
import pspec_real_ref
import pspec_ref

SEED = 0x5EED0F5F
RUNGS = np.array([2.0 ** e for e in range(-84, -57, 2)] + [1.0] + [2.0 ** e for e in range(54, 71)] + [0.0, -0.0], np.float32)
assert len(RUNGS) == 34

# the polyphase spectrometer: (M, P, K, taps); the three 64-channel shapes with 4 / 8 / 16 taps per branch are the fused kernel
PFB = [(64, 16, 17, "lpf"), (64, 4, 5, "synth"), (64, 8, 1, "lpf"), (64, 16, 40, "synth"), (128, 8, 17, "lpf"), (100, 5, 5, "synth")]
PSPEC = [(1024, 17, 1024), (1024, 5, 512), (96, 17, 48), (4096, 2, 4096)]   # (N, K, step): PowerSpectrum
PSPEC_REAL = [(2048, 17, 2048), (2048, 5, 1024), (1000, 3, 1000)]           # PowerSpectrumReal


def ladder(x, H):
    """the first 34 blocks of 2 H samples of x (float32 or complex64), block b times RUNGS[b], every word multiplied in float32"""
    n = 2 * H * len(RUNGS)
    assert len(x) >= n
    y = x[:n].copy()
    w = y.view(np.float32).reshape(len(RUNGS), -1)
    w *= RUNGS[:, None]
    return y


def pfb_taps(oracle, M, P, taps):
    return oracle.lpf_corrected(M * P, 0.45 / M) if taps == "lpf" else oracle.synth_f32(9, P, M * P)


_made = {}


def case(oracle, kind, shape):
    """(input, taps or None, the restatement's rows) of one case, computed once"""
    key = (kind,) + tuple(shape)
    if key not in _made:
        with np.errstate(over="ignore"):   # the overflow is the point
            _made[key] = _make(oracle, kind, shape)
    return _made[key]


def _make(oracle, kind, shape):
    if kind == "pfb":
        M, P, K, taps = shape
        h = pfb_taps(oracle, M, P, taps)
        x = ladder(oracle.synth_iq(SEED, 0, 68 * K * M), K * M)
        return x, h, pfb_pspec_ref.spectrum(x, h, M, P, K, True)
    elif kind == "pspec":
        N, K, step = shape
        x = ladder(oracle.synth_iq(SEED, 0, 68 * K * step), K * step)
        return x, None, pspec_ref.power_spectrum(x, N, K, step)
    else:
        N, K, step = shape
        x = ladder(oracle.synth_f32(SEED, 0, 68 * K * step), K * step)
        return x, None, pspec_real_ref.power_spectrum(x, N, K, step)


def classes(want):
    """fractions of the outputs that are exact zeros, nonzero subnormals, inf, finite normal values, NaN"""
    a = np.abs(np.asarray(want, np.float32).reshape(-1))
    tiny = np.float32(2.0 ** -126)
    return {"zero": float((a == 0).mean()), "subnormal": float(((a > 0) & (a < tiny)).mean()), "inf": float(np.isinf(a).mean()),
            "normal": float((np.isfinite(a) & (a >= tiny)).mean()), "nan": float(np.isnan(a).mean())}
