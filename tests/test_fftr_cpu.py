"""The real-input transform without a GPU: the restatement (tests/fftr_ref.py) against numpy in float64, the kernels' thread and lane
programs (libredio_amd/csrc/fftr_core.h) emulated on the CPU bit for bit against the restatement, and the C ABI of the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fftr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [2, 4, 6, 8, 10, 14, 22, 30, 64, 128, 200, 486, 512, 1000, 2048, 4096, 8192, 16384, 32400, 32768, 131072]
BOUND = 2e-6  # the project's relative-L2 bound of a float32 transform against float64
c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rel_l2(got, want):
    got, want = np.asarray(got, np.complex128), np.asarray(want, np.complex128)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


@pytest.fixture(scope="module")
def emu_fftr():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_fftr"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_fftr.so"))
    E.emu_fftr_super_tw.argtypes = [C.c_int, C.c_int, c64]
    E.emu_fftr_split.argtypes = [C.c_int, C.c_int, c64, c64]
    E.emu_fftr1k_post.argtypes = [c64, c64]
    E.emu_fftr1k_pre.argtypes = [c64, c64]
    return E


@pytest.mark.parametrize("n", SIZES)
def test_restatement_against_numpy(oracle, n):
    x = oracle.synth_f32(0xF7 + n, 0, n)
    f = fftr_ref.fftr(x)
    e_f = rel_l2(f, np.fft.rfft(x.astype(np.float64)))
    assert f.imag[0] == 0 and not np.signbit(f.imag[0]) and f.imag[n // 2] == 0 and not np.signbit(f.imag[n // 2])
    g = oracle.synth_iq(0xF8 + n, 0, n // 2 + 1)
    t = fftr_ref.fftri(g)
    g64 = g.astype(np.complex128)
    g64.imag[0] = g64.imag[-1] = 0  # kiss_fftri ignores them; numpy's irfft does too, stated here for clarity
    e_i = rel_l2(t, np.fft.irfft(g64, n) * n)
    e_rt = rel_l2(fftr_ref.fftri(f), x.astype(np.float64) * n)
    print(f"N={n}: forward {e_f:.3g} inverse {e_i:.3g} round trip {e_rt:.3g}")
    assert e_f <= BOUND and e_i <= BOUND
    assert e_rt <= BOUND


def test_super_twiddles(emu_fftr):
    for M in (1, 2, 3, 5, 15, 64, 1024):
        for inv in (0, 1):
            tw = np.zeros(max(M // 2, 1), np.complex64)
            emu_fftr.emu_fftr_super_tw(M, inv, tw)
            want = fftr_ref.super_tw(M, bool(inv))
            assert [(c.real, c.imag) for c in tw[: M // 2]] == [(float(a), float(b)) for a, b in want]


@pytest.mark.parametrize("M", [1, 2, 3, 5, 15, 64, 1024])
def test_split_thread_programs(emu_fftr, oracle, M):
    """fftr_post_thread / fftr_pre_thread of the generic kernels, element by element over the oracle's complex transform."""
    x = oracle.synth_f32(0xA0 + M, 0, 2 * M)
    Z = oracle.fft(x.view(np.complex64)) if M > 1 else x.view(np.complex64).copy()
    f = np.full(M + 1, np.nan, np.complex64)
    assert emu_fftr.emu_fftr_split(M, 0, Z, f) == 1
    assert np.array_equal(bits(f), bits(fftr_ref.fftr(x)))
    g = oracle.synth_iq(0xB0 + M, 0, M + 1)
    T = np.full(M, np.nan, np.complex64)
    assert emu_fftr.emu_fftr_split(M, 1, g, T) == 1
    t = oracle.fft(T, inverse=True) if M > 1 else T
    assert np.array_equal(bits(t), bits(fftr_ref.fftri(g)))


def test_fused_lane_programs(emu_fftr, oracle):
    """The fused 2048-point kernels' split: sixty-four lanes with the one-wave transform's register layout and natural-order image."""
    assert emu_fftr.emu_fftr1k_map_ok() == 1
    x = oracle.synth_f32(0xC1, 0, 2048)
    Z = oracle.fft(x.view(np.complex64))
    f = np.full(1025, np.nan, np.complex64)
    assert emu_fftr.emu_fftr1k_post(Z, f) == 1
    assert np.array_equal(bits(f), bits(fftr_ref.fftr(x)))
    g = oracle.synth_iq(0xC2, 0, 1025)
    T = np.full(1024, np.nan, np.complex64)
    assert emu_fftr.emu_fftr1k_pre(g, T) == 1
    assert np.array_equal(bits(oracle.fft(T, inverse=True)), bits(fftr_ref.fftri(g)))


REDIO_FFTR = ["redio_fftr_create", "redio_fftr_destroy", "redio_fftr_reserve", "redio_fftr_is_fused", "redio_fftr_enqueue",
              "redio_fftr_enqueue_strided"]
KISS_FFTR = ["kiss_fftr_alloc", "kiss_fftr", "kiss_fftri", "kiss_fftr_free"]


def test_abi(redio, capfd):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_fftr redio_fftr;" in hdr  # the seventh name of the interface: the opaque handle type
    for n in REDIO_FFTR:
        assert hasattr(L, n), f"libredio.so does not export {n}"
        assert n + "(" in hdr
    K = redio.kisslib()
    for n in KISS_FFTR:
        assert hasattr(K, n), f"libkissfft.so does not export {n}"
    h = os.path.join(ROOT, "include", "kiss_fftr.h")
    for cc, std, lang in (("gcc", "-std=c99", "c"), ("g++", "-std=c++17", "c++")):
        r = subprocess.run([cc, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-x", lang, h], capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (cc, r.stderr)
    p = C.c_void_p()
    assert redio.lib().redio_fftr_create(C.byref(p), 7, 0) == -1 and redio.lib().redio_fftr_create(C.byref(p), 0, 0) == -1
    assert redio.lib().redio_fftr_create(None, 64, 0) == -1
    assert K.kiss_fftr_alloc(7, 0, None, None) is None
    assert "Real FFT optimization must be even." in capfd.readouterr().err


def test_no_device_no_fallback(redio):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    assert redio.lib().redio_fftr_create(C.byref(p), 64, 0) == -4 and not p.value
    assert redio.kisslib().kiss_fftr_alloc(64, 0, None, None) is None
    assert redio.kisslib().kiss_fftr_alloc(7, 0, None, None) is None
