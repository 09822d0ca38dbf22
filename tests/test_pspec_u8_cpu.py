"""The integrated power spectrum from the receiver's u8 I/Q bytes (redio_pspec_enqueue_u8) without a GPU: the fused
u8 kernel's sixty-four lane programs and the generic gather's thread program (libredio_amd/csrc/pspec_core.h) emulated on the CPU bit
for bit against pspec_ref.power_spectrum(oracle.data_to_samples(bytes), ...), the conversion on all 256 byte values, and the C ABI of
the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pspec_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0B5C


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


@pytest.fixture(scope="module")
def emu_u8():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pspec_u8"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pspec_u8.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    E.emu_pspec1k_u8.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_int, C.c_long, f32, i32]
    E.emu_pspec1k_u8.restype = None
    E.emu_pspec_rows_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_long, c64, i32]
    E.emu_pspec_rows_u8.restype = None
    E.emu_i2f_all.argtypes = [f32]
    E.emu_i2f_all.restype = None
    return E


def test_conversion_on_all_256_bytes(emu_u8, oracle):
    """i2f as the host compiles it (the emulation's conversion) against the oracle's i as f32 / 127.0 - 1.0"""
    got = np.empty(256, np.float32)
    emu_u8.emu_i2f_all(got)
    b = np.arange(256, dtype=np.uint8)
    want = oracle.data_to_samples(np.stack([b, b[::-1]], axis=1).reshape(-1))
    assert np.array_equal(bits(got), bits(want.real.copy()))
    assert np.array_equal(bits(got[::-1].copy()), bits(want.imag.copy()))


@pytest.fixture(scope="module")
def fused_cases(oracle):
    """per (K, step): two rows' worth of bytes (and five samples more) at byte offset 2 of a buffer, and the checker's rows with and
    without the window, computed once"""
    w = oracle.lpf_corrected(1024, 0.1)
    made = {}
    for K in (1, 16, 17, 40):
        for step in (1024, 512, 1000):
            W, H = ref.shape(1024, K, step)
            buf = random_bytes(SEED + 64 * K + step, 2 + 2 * (W + H + 5))
            x = oracle.data_to_samples(buf[2:])
            made[(K, step)] = (buf, {False: ref.power_spectrum(x, 1024, K, step, None), True: ref.power_spectrum(x, 1024, K, step, w)})
    return w, made


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("step", [1024, 512, 1000])
@pytest.mark.parametrize("K", [1, 16, 17, 40])
def test_fused_u8_lane_programs(emu_u8, fused_cases, K, step, windowed):
    """Two rows through the sixty-four lanes of pspec1k_u8_kernel's program, one wave per row (row mode) and one wave per segment
    (segment mode, then the fold): load of the raw words (with the prefetch of the next transform's), convert, window, transform
    passes, square, both folds, stores -- bit for bit against the checker, every output element written exactly once.  The bytes
    start at byte offset 2 of their buffer."""
    N, rows = 1024, 2
    w, made = fused_cases
    buf, wants = made[(K, step)]
    want = wants[windowed]
    assert want.shape == (rows, N)
    base = buf.ctypes.data + 2
    wp = w.ctypes.data_as(C.c_void_p) if windowed else None
    out = np.full((rows, N), np.nan, np.float32)
    stores = np.zeros(rows * N, np.int32)
    emu_u8.emu_pspec1k_u8(base, step, K, wp, 0, rows, out.reshape(-1), stores)
    assert (stores == 1).all()
    assert np.array_equal(bits(out), bits(want))
    S = -(-K // ref.SEG)
    part = np.full((rows * S, N), np.nan, np.float32)
    stores = np.zeros(rows * S * N, np.int32)
    emu_u8.emu_pspec1k_u8(base, step, K, wp, 1, rows * S, part.reshape(-1), stores)
    assert (stores == 1).all()
    if S == 1:
        assert np.array_equal(bits(part), bits(want))  # the two modes coincide: no fold
    else:
        folded = part.reshape(rows, S, N)[:, 0].copy()
        for s in range(1, S):
            folded = folded + part.reshape(rows, S, N)[:, s]
        assert np.array_equal(bits(folded), bits(want))


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("N,K,step,nrows", [(64, 33, 64, 2), (1000, 5, 1000, 2), (15, 3, 7, 2), (15, 3, 7, 1)])
def test_generic_gather_thread_program(emu_u8, oracle, N, K, step, nrows, windowed):
    """pspec_rows_u8_kernel's lane steps (two consecutive elements each) over the rows' K transforms: the packed rows are the
    converted (and windowed) samples, each written once; transformed and integrated they are the checker's rows.  At N = 15 a step's
    second element opens the next row, and one row of three transforms is an odd count: the last element goes on its own."""
    W, H = ref.shape(N, K, step)
    raw = random_bytes(SEED + N, 2 * (W + (nrows - 1) * H))
    w = oracle.lpf_corrected(N, 0.1) if windowed else None
    x = oracle.data_to_samples(raw)
    ntr = nrows * K
    rows = np.full(ntr * N, np.nan + 0j, np.complex64)
    stores = np.zeros(ntr * N, np.int32)
    emu_u8.emu_pspec_rows_u8(raw.ctypes.data, w.ctypes.data_as(C.c_void_p) if windowed else None, ntr, N, step, rows, stores)
    assert (stores == 1).all()
    want_rows = np.stack([x[t * step: t * step + N] for t in range(ntr)])
    if windowed:
        xw = np.empty_like(want_rows)
        xw.real, xw.imag = want_rows.real * w, want_rows.imag * w
        want_rows = xw
    assert np.array_equal(np.ascontiguousarray(rows).view(np.uint32), np.ascontiguousarray(want_rows).reshape(-1).view(np.uint32))
    got = ref.spectra(oracle.fft(rows, N), N, K)
    assert np.array_equal(bits(got), bits(ref.power_spectrum(x, N, K, step, w)))


NAMES = ["redio_pspec_enqueue_u8", "redio_pspec_reserve_u8", "redio_pspec_stream_create_u8"]


def test_abi_u8(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    for n in NAMES:
        assert hasattr(L, n), f"libredio.so does not export {n}"
        assert n + "(" in hdr
    R = redio.lib()
    assert R.redio_pspec_enqueue_u8(None, None, 4096, None, None) == -1
    assert R.redio_pspec_reserve_u8(None, 4096) == -1
    p = C.c_void_p(1)
    assert R.redio_pspec_stream_create_u8(C.byref(p), None) == -1 and not p.value
    assert R.redio_pspec_stream_create_u8(None, None) == -1
    assert hasattr(redio.PowerSpectrum, "u8") and hasattr(redio.PowerSpectrum, "reserve_u8")


def test_no_device_no_fallback_u8(redio):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    assert redio.lib().redio_pspec_create(C.byref(p), 1024, 4, 1024, None) == -4 and not p.value
