"""The real-input integrated power spectrum without a GPU: the restatement (tests/pspec_real_ref.py) against float64, the row-count
laws, the fused 2048-point kernel's lane programs and the generic path's thread programs (libredio_amd/csrc/pspec_real_core.h)
emulated on the CPU bit for bit against the restatement, and the C ABI of the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fftr_ref
import pspec_real_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0B5D
# (N, K, step, windowed)
SHAPES = [(2, 3, 2, False), (6, 2, 6, False), (64, 33, 64, True), (1000, 5, 1000, True), (2048, 17, 2048, False),
          (2048, 17, 1024, True), (2048, 40, 2000, True), (4096, 4, 1000, True), (2050, 3, 2050, False)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("N,K,step,windowed", SHAPES)
def test_restatement_against_float64(oracle, N, K, step, windowed):
    """two rows of oracle.synth_f32 input against float64 sum |numpy.fft.rfft|^2; max|got - exact| / max(exact) <= 2e-6, the
    project's FFT bound (measured on these shapes: 2.9e-8 ... 2.6e-7)"""
    W, H = ref.shape(N, K, step)
    x = oracle.synth_f32(SEED, 0, W + H)
    w = oracle.lpf_corrected(N, 0.1) if windowed else None
    got = ref.power_spectrum(x, N, K, step, w)
    assert got.shape == (2, N // 2 + 1) and got.dtype == np.float32
    x64 = x.astype(np.float64)
    exact = np.zeros((2, N // 2 + 1))
    for r in range(2):
        for t in range(K):
            seg = x64[(r * K + t) * step: (r * K + t) * step + N]
            exact[r] += np.abs(np.fft.rfft(seg * w.astype(np.float64) if windowed else seg)) ** 2
    err = float(np.abs(got - exact).max() / exact.max())
    print(f"N={N} K={K} step={step} window={windowed}: distance from float64 {err:.3g}, bound 2e-06")
    assert err <= 2e-6


@pytest.mark.parametrize("N,K,step", [(2048, 1, 2048), (2048, 17, 1024), (64, 33, 64), (4096, 4, 1000), (6, 2, 6), (2, 3, 2), (16, 3, 40),
                                      (2048, 5, 3000)])
def test_nrows_laws(N, K, step):
    W, H = ref.shape(N, K, step)
    assert (W, H) == ((K - 1) * step + N, K * step)
    assert ref.nrows(W - 1, N, K, step) == 0 and ref.nrows(W, N, K, step) == 1
    assert ref.nrows(W + H - 1, N, K, step) == 1 and ref.nrows(W + H, N, K, step) == 2
    assert ref.nrows(0, N, K, step) == 0 and ref.nrows(W + 9 * H, N, K, step) == 10
    assert ref.nbins(N) == N // 2 + 1


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pspec_real"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pspec_real.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    E.emu_pspecr2k.argtypes = [f32, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_long, f32, i32]
    E.emu_pspecr2k.restype = None
    E.emu_pspec_real_rows.argtypes = [f32, C.c_void_p, C.c_long, C.c_long, C.c_long, f32, i32]
    E.emu_pspec_real_rows.restype = None
    E.emu_pspec_real_generic.argtypes = [c64, C.c_long, C.c_long, C.c_long, f32, f32, i32, i32]
    E.emu_pspec_real_generic.restype = None
    return E


_want = {}


def fused_case(oracle, K, step, windowed):
    """the input (8-byte aligned), the window and the restatement's rows of one fused shape, computed once"""
    key = (K, step, windowed)
    if key not in _want:
        N, rows = 2048, 2
        W, H = ref.shape(N, K, step)
        x = oracle.synth_f32(SEED + K, 0, W + (rows - 1) * H + 5)
        w = oracle.lpf_corrected(N, 0.1) if windowed else None
        want = ref.power_spectrum(x, N, K, step, w)
        assert want.shape == (rows, N // 2 + 1)
        want.setflags(write=False)
        _want[key] = (x, w, want)
    return _want[key]


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("step", [2048, 1024, 1001])
@pytest.mark.parametrize("K", [1, 16, 17, 40])
def test_fused_lane_programs(emu, oracle, K, step, windowed):
    """Two rows through the sixty-four lanes of pspecr2k_kernel's program, one wave per row and one wave per segment (and the fold
    thread program): load in both forms, window, transform passes, LDS image, split, square, segment and row folds, stores -- bit
    for bit against the restatement, every one of the rows * 1025 output elements written exactly once."""
    N, B, rows = 2048, 1025, 2
    x, w, want = fused_case(oracle, K, step, windowed)
    wp = w.ctypes.data_as(C.c_void_p) if windowed else None
    assert x.ctypes.data % 8 == 0
    forms = [0] + ([1] if step % 2 == 0 else [])  # the 8-byte form only where the launcher would pick it
    for pairs in forms:
        out = np.full((rows, B), np.nan, np.float32)
        stores = np.zeros(rows * B, np.int32)
        emu.emu_pspecr2k(x, step, K, wp, 0, pairs, rows, out.reshape(-1), stores)
        assert (stores == 1).all()
        assert np.array_equal(bits(out), bits(want)), f"pairs={pairs}"
    S = -(-K // ref.SEG)
    part = np.full((rows * S, B), np.nan, np.float32)
    stores = np.zeros(rows * S * B, np.int32)
    emu.emu_pspecr2k(x, step, K, wp, 1, forms[-1], rows * S, part.reshape(-1), stores)
    assert (stores == 1).all()
    if S == 1:
        assert np.array_equal(bits(part), bits(want))  # the two modes coincide: no fold
    else:
        folded = part.reshape(rows, S, B)[:, 0].copy()
        for s in range(1, S):
            folded = folded + part.reshape(rows, S, B)[:, s]
        assert np.array_equal(bits(folded), bits(want))


def test_fused_unaligned_base(emu, oracle):
    """a stream that starts one float into its buffer (4-byte aligned only) takes the two-float load form: the same bits"""
    K, step = 3, 2048
    W, H = ref.shape(2048, K, step)
    buf = oracle.synth_f32(SEED, 0, W + H + 1)
    x = buf[1:]
    assert x.ctypes.data % 8 == 4
    want = ref.power_spectrum(x, 2048, K, step)
    out = np.full((2, 1025), np.nan, np.float32)
    stores = np.zeros(2 * 1025, np.int32)
    emu.emu_pspecr2k(x, step, K, None, 0, 0, 2, out.reshape(-1), stores)
    assert (stores == 1).all() and np.array_equal(bits(out), bits(want))


@pytest.mark.parametrize("N,K", [(64, 33), (1000, 3), (6, 33), (2050, 3)])
@pytest.mark.parametrize("windowed", [False, True])
def test_generic_thread_programs(emu, oracle, N, K, windowed):
    """the row gather's threads (overlapping rows, with and without a window), then the accumulate and fold threads over the
    restatement's kiss_fftr rows of N / 2 + 1 bins (an even count at N = 1000, 6 and 2050, where M is odd or B is even)"""
    rows, B = 2, N // 2 + 1
    step = N - 3 if N > 6 else N
    W, H = ref.shape(N, K, step)
    x = oracle.synth_f32(SEED + N, 0, W + (rows - 1) * H + 3)
    w = oracle.lpf_corrected(N, 0.1) if windowed else None
    want_rows = ref.gather(x, N, K, step, w)
    ntr = rows * K
    got_rows = np.full(ntr * N, np.nan, np.float32)
    sr = np.zeros(ntr * N, np.int32)
    emu.emu_pspec_real_rows(x, w.ctypes.data_as(C.c_void_p) if windowed else None, ntr, N, step, got_rows, sr)
    assert (sr == 1).all()
    assert np.array_equal(bits(got_rows.reshape(ntr, N)), bits(want_rows))
    X = np.ascontiguousarray(fftr_ref.fftr_rows(want_rows, N))
    want = ref.power_spectrum(x, N, K, step, w)
    assert np.array_equal(bits(ref.spectra(X, N, K)), bits(want))
    S = -(-K // ref.SEG)
    part = np.full(rows * S * B, np.nan, np.float32)
    out = np.full(rows * B, np.nan, np.float32)
    sp, so = np.zeros(rows * S * B, np.int32), np.zeros(rows * B, np.int32)
    emu.emu_pspec_real_generic(X.reshape(-1), B, K, rows, part, out, sp, so)
    assert (sp == 1).all() and (so == 1).all()
    assert np.array_equal(bits(out.reshape(rows, B)), bits(want))
    if S == 1:
        assert np.array_equal(bits(part), bits(out))  # K <= 16: the accumulate pass writes the rows


NAMES = ["redio_pspec_real_create", "redio_pspec_real_destroy", "redio_pspec_real_nrows", "redio_pspec_real_nbins",
         "redio_pspec_real_is_fused", "redio_pspec_real_reserve", "redio_pspec_real_enqueue", "redio_pspec_real_enqueue_spectra",
         "redio_pspec_real_set_split"] + [
             f"redio_pspec_real_stream_{s}" for s in ("create", "destroy", "reset", "nout", "pending", "enqueue")]


def test_abi(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_pspec_real redio_pspec_real;" in hdr
    assert "typedef struct redio_pspec_real_stream redio_pspec_real_stream;" in hdr
    for n in NAMES:
        assert hasattr(L, n), f"libredio.so does not export {n}"
        assert n + "(" in hdr
    doc = hdr[hdr.index("the real-input integrated power spectrum"): hdr.index("typedef struct redio_pspec_real ")]
    assert "tools/kiss_fftr.c" in doc and "DESIGN.md 5.3c" in doc and "4 N / step" in doc and "N = 2048 is ONE kernel" in doc
    R = redio.lib()
    p = C.c_void_p()
    w = (C.c_float * 2048)(*([0.5] * 2048))
    assert R.redio_pspec_real_create(None, 2048, 4, 2048, None) == -1
    assert R.redio_pspec_real_create(C.byref(p), 0, 4, 2048, None) == -1 and R.redio_pspec_real_create(C.byref(p), -6, 4, 2048, w) == -1
    assert R.redio_pspec_real_create(C.byref(p), 2047, 4, 2048, None) == -1  # odd
    assert R.redio_pspec_real_create(C.byref(p), 1, 4, 1, None) == -1
    assert R.redio_pspec_real_create(C.byref(p), 2048, 0, 2048, None) == -1
    assert R.redio_pspec_real_create(C.byref(p), 2048, 4, 0, w) == -1
    assert R.redio_pspec_real_create(C.byref(p), (1 << 25) + 2, 4, 2048, None) == -3  # redio_fftr_create's ceiling
    assert not p.value
    assert R.redio_pspec_real_nrows(None, 1 << 20) == 0 and R.redio_pspec_real_is_fused(None) == 0 and R.redio_pspec_real_nbins(None) == 0
    assert R.redio_pspec_real_destroy(None) == 0
    assert R.redio_pspec_real_reserve(None, 4096) == -1 and R.redio_pspec_real_set_split(None, 1) == -1
    assert R.redio_pspec_real_enqueue(None, None, 4096, None, None) == -1
    assert R.redio_pspec_real_enqueue_spectra(None, None, 4, None, None) == -1
    assert R.redio_pspec_real_stream_create(C.byref(p), None) == -1 and R.redio_pspec_real_stream_create(None, None) == -1
    assert R.redio_pspec_real_stream_nout(None, 5) == 0 and R.redio_pspec_real_stream_pending(None) == 0
    assert R.redio_pspec_real_stream_reset(None) == -1 and R.redio_pspec_real_stream_destroy(None) == 0
    assert R.redio_pspec_real_stream_enqueue(None, None, 5, None, None, None) == -1


def test_no_device_no_fallback(redio):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    assert redio.lib().redio_pspec_real_create(C.byref(p), 2048, 4, 2048, None) == -4 and not p.value
    with pytest.raises(redio.RedioError):
        redio.PowerSpectrumReal(2048, 4)
