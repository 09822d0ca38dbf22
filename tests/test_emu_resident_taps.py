"""The chain kernels' FIR lane programs on the CPU (tests/emu_taps: the host path of libredio_amd/csrc/fir_core.h): the resident-taps
program (fir_lane_v_res: ceil(K/2) values, tap j = element min(j, K-1-j), samples ascending, live outputs in turn) against the staged
program (fir_lane_v) and against oracle.fir, bit for bit, on random mirrored taps whose values are all distinct -- a tap map or a live
range that is off by one changes bits."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(127, 5), (63, 5), (127, 3), (127, 1), (63, 1), (64, 2), (7, 2)]
LANES = 5


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def emu_taps():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_taps"), "-s"])
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_taps.so"))
    pf = C.POINTER(C.c_float)
    lib.emu_taps_fir.argtypes = [C.c_int, C.c_int, C.c_int, pf, pf, C.c_int, pf, pf]
    lib.emu_taps_fir.restype = C.c_int
    return lib


def mirrored_taps(k):
    rng = np.random.default_rng(0x7A95 + k)
    half = rng.uniform(-0.5, 0.5, (k + 1) // 2).astype(np.float32)
    assert len(np.unique(bits(half))) == len(half)
    t = np.empty(k, np.float32)
    t[: len(half)] = half
    t[k - len(half):] = half[::-1]
    assert np.array_equal(bits(t), bits(t[::-1]))
    return t


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_resident_program_matches_staged_and_oracle(emu_taps, oracle, k, d, fused):
    pf = C.POINTER(C.c_float)
    taps = mirrored_taps(k)
    nout = 4 * LANES
    x = oracle.synth_iq(0x7AB5 + k + d, 0, (nout - 1) * d + k)
    staged, res = np.zeros(nout, np.complex64), np.zeros(nout, np.complex64)
    rc = emu_taps.emu_taps_fir(k, d, int(fused), x.ctypes.data_as(pf), taps.ctypes.data_as(pf), LANES, staged.ctypes.data_as(pf), res.ctypes.data_as(pf))
    assert rc == 0
    want = oracle.fir(x, taps, d, fused=fused)
    assert want.shape == (nout,)
    assert np.array_equal(bits(staged), bits(want)), "the staged program differs from the oracle"
    assert np.array_equal(bits(res), bits(want)), "the resident program differs from the oracle"
