"""The integrated power spectrum without a GPU: the restatement (tests/pspec_ref.py) against float64, the row-count laws, the fused
kernel's lane programs and the generic passes' thread programs (libredio_amd/csrc/pspec_core.h) emulated on the CPU bit for bit
against the restatement, and the C ABI of the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pspec_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0B5C
# (N, K, step, windowed)
SHAPES = [(1024, 1, 1024, False), (1024, 3, 1024, True), (1024, 16, 1024, False), (1024, 17, 1024, True), (1024, 40, 512, True),
          (1024, 100, 1024, False), (64, 33, 64, False), (1000, 5, 1000, True), (2048, 20, 2048, False), (4096, 4, 1000, True),
          (6, 2, 6, False)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N,K,step,windowed", SHAPES)
def test_restatement_against_float64(oracle, N, K, step, windowed):
    """two rows of oracle.synth_iq input; max|got - exact| / max(exact) <= 2e-6, the project's FFT bound (measured: 8.4e-8 ... 3.1e-7)"""
    W, H = ref.shape(N, K, step)
    x = oracle.synth_iq(SEED, 0, W + H)
    w = oracle.lpf_corrected(N, 0.1) if windowed else None
    got = ref.power_spectrum(x, N, K, step, w)
    assert got.shape == (2, N) and got.dtype == np.float32
    x64 = x.astype(np.complex128)
    exact = np.zeros((2, N))
    for r in range(2):
        for t in range(K):
            seg = x64[(r * K + t) * step: (r * K + t) * step + N]
            exact[r] += np.abs(np.fft.fft(seg * w.astype(np.float64) if windowed else seg)) ** 2
    err = float(np.abs(got - exact).max() / exact.max())
    print(f"N={N} K={K} step={step} window={windowed}: distance from float64 {err:.3g}, bound 2e-06")
    assert err <= 2e-6


@pytest.mark.parametrize("N,K,step", [(1024, 1, 1024), (1024, 17, 512), (64, 33, 64), (4096, 4, 1000), (6, 2, 6), (16, 3, 40)])
def test_nrows_laws(N, K, step):
    W, H = ref.shape(N, K, step)
    assert (W, H) == ((K - 1) * step + N, K * step)
    assert ref.nrows(W - 1, N, K, step) == 0 and ref.nrows(W, N, K, step) == 1
    assert ref.nrows(W + H - 1, N, K, step) == 1 and ref.nrows(W + H, N, K, step) == 2
    assert ref.nrows(0, N, K, step) == 0 and ref.nrows(W + 9 * H, N, K, step) == 10


@pytest.fixture(scope="module")
def emu_pspec():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pspec"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pspec.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    E.emu_pspec1k.argtypes = [c64, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_long, f32, i32]
    E.emu_pspec1k.restype = None
    E.emu_pspec_generic.argtypes = [c64, C.c_long, C.c_long, C.c_long, f32, f32, i32, i32]
    E.emu_pspec_generic.restype = None
    return E


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("K,step", [(1, 1024), (16, 1024), (17, 1000), (40, 512)])
def test_fused_lane_programs(emu_pspec, oracle, K, step, windowed):
    """Two rows through the sixty-four lanes of pspec1k_kernel's program, one wave per row and one wave per segment (and the fold
    thread program): load, window, transform passes, square, segment and row folds, stores -- bit for bit against the restatement,
    every output element written exactly once."""
    N, rows = 1024, 2
    W, H = ref.shape(N, K, step)
    x = oracle.synth_iq(SEED + K, 0, W + (rows - 1) * H + 5)
    w = oracle.lpf_corrected(N, 0.1) if windowed else None
    want = ref.power_spectrum(x, N, K, step, w)
    assert want.shape == (rows, N)
    wp = w.ctypes.data_as(C.c_void_p) if windowed else None
    out = np.full((rows, N), np.nan, np.float32)
    stores = np.zeros(rows * N, np.int32)
    emu_pspec.emu_pspec1k(x, step, K, wp, 0, rows, out.reshape(-1), stores)
    assert (stores == 1).all()
    assert np.array_equal(bits(out), bits(want))
    S = -(-K // ref.SEG)
    part = np.full((rows * S, N), np.nan, np.float32)
    stores = np.zeros(rows * S * N, np.int32)
    emu_pspec.emu_pspec1k(x, step, K, wp, 1, rows * S, part.reshape(-1), stores)
    assert (stores == 1).all()
    if S == 1:
        assert np.array_equal(bits(part), bits(want))  # the two modes coincide: no fold
    else:
        folded = part.reshape(rows, S, N)[:, 0].copy()
        for s in range(1, S):
            folded = folded + part.reshape(rows, S, N)[:, s]
        assert np.array_equal(bits(folded), bits(want))


@pytest.mark.parametrize("N,K", [(64, 3), (64, 33), (1000, 3), (6, 33)])
def test_generic_thread_programs(emu_pspec, oracle, N, K):
    rows = 3
    X = oracle.fft(oracle.synth_iq(SEED + N, 0, rows * K * N), N)
    want = ref.spectra(X, N, K)
    S = -(-K // ref.SEG)
    part = np.full(rows * S * N, np.nan, np.float32)
    out = np.full(rows * N, np.nan, np.float32)
    sp, so = np.zeros(rows * S * N, np.int32), np.zeros(rows * N, np.int32)
    emu_pspec.emu_pspec_generic(X, N, K, rows, part, out, sp, so)
    assert (sp == 1).all() and (so == 1).all()
    assert np.array_equal(bits(out.reshape(rows, N)), bits(want))
    if S == 1:
        assert np.array_equal(bits(part), bits(out))  # K <= 16: the accumulate pass writes the rows


NAMES = ["redio_pspec_create", "redio_pspec_destroy", "redio_pspec_nrows", "redio_pspec_is_fused", "redio_pspec_reserve",
         "redio_pspec_enqueue", "redio_pspec_enqueue_spectra", "redio_pspec_set_split"] + [
             f"redio_pspec_stream_{s}" for s in ("create", "destroy", "reset", "nout", "pending", "enqueue")]


def test_abi(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_pspec redio_pspec;" in hdr and "typedef struct redio_pspec_stream redio_pspec_stream;" in hdr
    assert "#define REDIO_PSPEC_SEG 16" in hdr
    for n in NAMES:
        assert hasattr(L, n), f"libredio.so does not export {n}"
        assert n + "(" in hdr
    doc = hdr[hdr.index("the integrated power spectrum"): hdr.index("typedef struct redio_pspec ")]
    assert "kissfft.rs:18-31" in doc and "NEW" in doc
    R = redio.lib()
    p = C.c_void_p()
    w = (C.c_float * 1024)(*([0.5] * 1024))
    assert R.redio_pspec_create(None, 1024, 4, 1024, None) == -1
    assert R.redio_pspec_create(C.byref(p), 0, 4, 1024, None) == -1 and R.redio_pspec_create(C.byref(p), -5, 4, 1024, w) == -1
    assert R.redio_pspec_create(C.byref(p), 1024, 0, 1024, None) == -1
    assert R.redio_pspec_create(C.byref(p), 1024, 4, 0, w) == -1
    assert R.redio_pspec_create(C.byref(p), (1 << 26) + 1, 4, 1024, None) == -3  # redio_fft_create's ceiling
    assert not p.value
    assert R.redio_pspec_nrows(None, 1 << 20) == 0 and R.redio_pspec_is_fused(None) == 0
    assert R.redio_pspec_destroy(None) == 0
    assert R.redio_pspec_reserve(None, 4096) == -1 and R.redio_pspec_set_split(None, 1) == -1
    assert R.redio_pspec_enqueue(None, None, 4096, None, None) == -1 and R.redio_pspec_enqueue_spectra(None, None, 4, None, None) == -1
    assert R.redio_pspec_stream_create(C.byref(p), None) == -1 and R.redio_pspec_stream_create(None, None) == -1
    assert R.redio_pspec_stream_nout(None, 5) == 0 and R.redio_pspec_stream_pending(None) == 0
    assert R.redio_pspec_stream_reset(None) == -1 and R.redio_pspec_stream_destroy(None) == 0
    assert R.redio_pspec_stream_enqueue(None, None, 5, None, None, None) == -1


def test_no_device_no_fallback(redio):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    assert redio.lib().redio_pspec_create(C.byref(p), 1024, 4, 1024, None) == -4 and not p.value
    with pytest.raises(redio.RedioError):
        redio.PowerSpectrum(1024, 4)
