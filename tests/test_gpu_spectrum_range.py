"""The range edges of the power stage on the GPU: re * re + im * im and the blocked sum of DESIGN.md 5.3c on the amplitude ladder of
tests/spectrum_ladder.py, whose outputs are exact zeros, subnormals, normal values and inf in comparable shares
(tests/test_spectrum_range_cpu.py) and never NaN.  The polyphase spectrometer's power tile and fold, the fused 1024- and 2048-point
kernels, and the generic accumulate and fold passes, bit for bit against the restatements: a power stage that flushes subnormals, or
a sum kept in a wider type that overflows later than float32 does, fails here and nowhere else."""
import numpy as np
import pytest

import spectrum_ladder as sl

pytestmark = pytest.mark.gpu

AUTO, ROWS, SEGMENTS = 0, 1, 2


def differing(got, want):
    """rows whose bits differ, with the first differing values"""
    g, w = np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)
    bad = np.argwhere(g != w)
    return [(int(r), int(c), float(got[r, c]), float(want[r, c])) for r, c in bad[:6]], len(bad)


def modes_of(K, fused, always=False):
    """fused polyphase shapes run every split mode; K = 17 plans the two explicit ones; the rest run as created"""
    return (AUTO, ROWS, SEGMENTS) if always and fused else (ROWS, SEGMENTS) if K == 17 else (AUTO,)


def compare(gpu, plan, x, want, modes):
    d = gpu.from_numpy(x).cuda()
    assert not np.isnan(want).any()
    for mode in modes:
        plan.set_split(mode)
        out = gpu.full((want.size + want.shape[1],), float("nan"), dtype=gpu.float32, device="cuda")
        got = plan(d, out=out).cpu().numpy()
        assert got.shape == want.shape, mode
        first, count = differing(got, want)
        assert not count, (mode, count, first)
        assert bool(out[want.size:].isnan().all()), mode


@pytest.mark.parametrize("M,P,K,taps", sl.PFB)
def test_polyphase_spectrum_on_the_ladder(gpu, redio, oracle, M, P, K, taps):
    x, h, want = sl.case(oracle, "pfb", (M, P, K, taps))
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    assert plan.is_fused == (M == 64)
    compare(gpu, plan, x, want, modes_of(K, plan.is_fused, always=True))


@pytest.mark.parametrize("N,K,step", sl.PSPEC)
def test_power_spectrum_on_the_ladder(gpu, redio, oracle, N, K, step):
    x, _, want = sl.case(oracle, "pspec", (N, K, step))
    plan = redio.PowerSpectrum(N, K, step)
    assert plan.is_fused == (N == 1024)
    compare(gpu, plan, x, want, modes_of(K, plan.is_fused))


@pytest.mark.parametrize("N,K,step", sl.PSPEC_REAL)
def test_power_spectrum_real_on_the_ladder(gpu, redio, oracle, N, K, step):
    x, _, want = sl.case(oracle, "pspec_real", (N, K, step))
    plan = redio.PowerSpectrumReal(N, K, step)
    assert plan.is_fused == (N == 2048)
    compare(gpu, plan, x, want, modes_of(K, plan.is_fused))
