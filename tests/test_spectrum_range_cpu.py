"""The amplitude ladder of tests/spectrum_ladder.py reaches every class of float32 in the restatements' outputs: what keeps
tests/test_gpu_spectrum_range.py from comparing nothing but inf, or nothing but normal values.  Conditions on the restatements alone,
not tolerances: each case has at least 5 % exact zeros, 5 % nonzero subnormals, 5 % inf and 25 % finite normal values, and no NaN."""
import numpy as np
import pytest

import spectrum_ladder as sl

CASES = [("pfb", s) for s in sl.PFB] + [("pspec", s) for s in sl.PSPEC] + [("pspec_real", s) for s in sl.PSPEC_REAL]


def test_the_rungs():
    r = sl.RUNGS
    assert len(r) == 34 and r.dtype == np.float32
    assert list(r[:14]) == [2.0 ** e for e in range(-84, -57, 2)] and r[14] == 1.0 and list(r[15:32]) == [2.0 ** e for e in range(54, 71)]
    assert r[32] == 0 and r[33] == 0 and not np.signbit(r[32]) and np.signbit(r[33])
    y = sl.ladder(np.ones(4 * 34, np.float32), 2)
    assert np.array_equal(y.view(np.uint32), np.repeat(r, 4).view(np.uint32))
    z = sl.ladder(np.full(2 * 34, 1 - 1j, np.complex64), 1)
    assert np.array_equal(z.real.view(np.uint32), np.repeat(r, 2).view(np.uint32)) and np.array_equal(z.imag.view(np.uint32), np.repeat(-r, 2).view(np.uint32))


@pytest.mark.parametrize("kind,shape", CASES)
def test_every_class_of_float32_is_in_the_restatements_rows(oracle, kind, shape):
    x, _, want = sl.case(oracle, kind, shape)
    assert np.isfinite(x.view(np.float32)).all()
    f = sl.classes(want)
    print(kind, shape, want.shape, {k: round(v, 3) for k, v in f.items()})
    assert f["nan"] == 0 and f["zero"] >= 0.05 and f["subnormal"] >= 0.05 and f["inf"] >= 0.05 and f["normal"] >= 0.25, f
