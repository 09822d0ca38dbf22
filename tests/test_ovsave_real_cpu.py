"""Overlap-save on real streams without a GPU: the restatement (tests/ovsave_real_ref.py) against the direct fold, the fused block's lane
programs (libredio_amd/csrc/ovsave_real_core.h and the register-output split of fftr_core.h) emulated on the CPU bit for bit against
the restatement, and the C ABI of the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fftr_ref
import ovsave_real_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2048, 1), (2048, 2), (2048, 127), (2048, 700), (2048, 2047), (512, 63), (1000, 101), (6, 3), (4096, 1025), (65536, 8193)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def taps_of(oracle, k):
    return oracle.lpf_corrected(k, 0.02) if k > 1 else np.array([0.75], np.float32)


def bound(taps, N):
    return 2e-6 * np.abs(taps).sum() * np.sqrt(np.log2(N)) + 1e-7  # tests/test_gpu_overlap_save.py:27


@pytest.mark.parametrize("N,k", SHAPES)
def test_restatement_against_the_direct_fold(oracle, N, k):
    taps = taps_of(oracle, k)
    hop = N - (k | 1) + 1
    assert ref.shape(k, N) == (k | 1, hop) and hop % 2 == 0
    for n in (N, N + hop - 1, N + 2 * hop + 17):
        x = oracle.synth_f32(0x5EED0105, 0, n)
        got = ref.overlap_save_real(x, taps, N)
        assert len(got) == ref.nout(n, k, N) == ((n - N) // hop + 1) * hop
        direct = oracle.convolve(x, taps)[: len(got)]
        err = float(np.abs(got - direct).max())
        print(f"N={N} K={k} n={n}: distance {err:.3g}, bound {bound(taps, N):.3g}")
        assert err <= bound(taps, N)
    assert ref.nout(N - 1, k, N) == 0


@pytest.fixture(scope="module")
def emu_ovsr():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_ovsave_real"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_ovsave_real.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    E.emu_ovsave_real2k_block.argtypes = [f32, c64, C.c_long, f32, c64, c64, np.ctypeslib.ndpointer(np.int32, flags="C")]
    return E


@pytest.mark.parametrize("k", [127, 2])
def test_fused_block_lane_programs(emu_ovsr, oracle, k):
    """One 2048-sample block through the sixty-four lanes of the fused kernel's program: the split's registers, the product, the
    hand-over into the inverse split and the masked pair store, each bit for bit against the restatement."""
    N = 2048
    taps = taps_of(oracle, k)
    hop = ref.shape(k, N)[1]
    x = oracle.synth_f32(0xE0 + k, 0, N)
    hr, hi = ref.spectrum(taps, N)
    Hc = np.empty(N // 2 + 1, np.complex64)
    Hc.real, Hc.imag = hr, hi
    out = np.full(N, np.nan, np.float32)
    freq = np.full(N // 2 + 1, np.nan, np.complex64)
    prod = np.full(N // 2 + 1, np.nan, np.complex64)
    stores = np.zeros(N // 2, np.int32)
    assert emu_ovsr.emu_ovsave_real2k_block(x, Hc, hop, out, freq, prod, stores) == 1
    X = fftr_ref.fftr(x)
    assert np.array_equal(bits(freq), bits(X))
    assert np.array_equal(bits(prod), bits(ref.product(X, (hr, hi))))
    assert np.array_equal(stores[: hop // 2], np.ones(hop // 2, np.int32)) and not stores[hop // 2:].any()
    assert np.isnan(out[hop:]).all()  # nothing at or beyond hop
    assert np.array_equal(bits(out[:hop]), bits(ref.overlap_save_real(x, taps, N)))


NAMES = ["redio_ovsave_real_create", "redio_ovsave_real_destroy", "redio_ovsave_real_nout", "redio_ovsave_real_is_fused",
         "redio_ovsave_real_reserve", "redio_ovsave_real_enqueue"] + [f"redio_ovsave_real_stream_{s}" for s in
                                                                     ("create", "destroy", "reset", "nout", "pending", "enqueue")]


def test_abi(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_ovsave_real redio_ovsave_real;" in hdr and "typedef struct redio_ovsave_real_stream redio_ovsave_real_stream;" in hdr
    for n in NAMES:
        assert hasattr(L, n), f"libredio.so does not export {n}"
        assert n + "(" in hdr
    assert "dsputils.rs:30-32" in hdr[hdr.index("overlap-save on REAL streams"): hdr.index("typedef struct redio_ovsave_real ")]
    create = redio.lib().redio_ovsave_real_create
    p = C.c_void_p()
    t = (C.c_float * 4096)(*([0.25] * 4096))
    assert create(C.byref(p), t, 0, 2048) == -1       # no taps
    assert create(C.byref(p), t, 2048, 2048) == -1    # Ke = 2049 > N
    assert create(C.byref(p), t, 65, 64) == -1
    assert create(C.byref(p), t, 3, 7) == -1          # odd N
    assert create(C.byref(p), t, 1, 0) == -1 and create(C.byref(p), t, 1, 1) == -1
    assert create(C.byref(p), None, 3, 64) == -1 and create(None, t, 3, 64) == -1
    assert create(C.byref(p), t, 3, 1 << 26) == -3    # redio_fftr_create's ceiling
    assert not p.value
    assert redio.lib().redio_ovsave_real_nout(None, 4096) == 0 and redio.lib().redio_ovsave_real_is_fused(None) == 0
    assert redio.lib().redio_ovsave_real_stream_create(C.byref(p), None) == -1


def test_no_device_no_fallback(redio):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    t = (C.c_float * 3)(0.25, 0.5, 0.25)
    assert redio.lib().redio_ovsave_real_create(C.byref(p), t, 3, 64) == -4 and not p.value
    with pytest.raises(redio.RedioError):
        redio.OverlapSaveReal([0.25, 0.5, 0.25], 2048)
