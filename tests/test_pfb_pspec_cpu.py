"""The polyphase spectrometer without a GPU: the row-count laws, the restatement (tests/pfb_pspec_ref.py: oracle.pfb_channelizer, then
pspec_ref.spectra) on a tone, the fused kernel's lane programs behind the transform (libredio_amd/csrc/pfb_pspec_core.h: the power
tile, the fold state machine, the stores) emulated on the CPU bit for bit against the restatement, and the C ABI of the new symbols."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pfb_pspec_ref as ref
import pspec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0F5C


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("M,P,K", [(64, 16, 1), (64, 4, 17), (128, 8, 40), (7, 2, 3), (1, 1, 1)])
def test_nrows_laws(M, P, K):
    W, H = ref.shape(M, P, K)
    assert (W, H) == ((K - 1 + P) * M, K * M)
    assert ref.nrows(W - 1, M, P, K) == 0 and ref.nrows(W, M, P, K) == 1
    assert ref.nrows(W + H - 1, M, P, K) == 1 and ref.nrows(W + H, M, P, K) == 2
    assert ref.nrows(0, M, P, K) == 0 and ref.nrows(W + 9 * H, M, P, K) == 10
    # the power spectrum's own law with a transform of P M samples every M
    assert pspec_ref.shape(M * P, K, M) == (W, H)


def test_restatement_is_the_composition(oracle):
    """K = 1 is re * re + im * im of the channelizer's rows; a trailing partial row is dropped"""
    h = oracle.synth_f32(9, 0, 64 * 4)
    x = oracle.synth_iq(SEED, 0, 64 * (4 - 1 + 11) + 3)
    rows = oracle.pfb_channelizer(x, h, 64, 4, False)
    assert len(rows) == 11
    got = ref.spectrum(x, h, 64, 4, 1)
    assert np.array_equal(bits(got), bits(rows.real * rows.real + rows.imag * rows.imag))
    got = ref.spectrum(x, h, 64, 4, 5)
    assert got.shape == (2, 64) and got.dtype == np.float32
    p = (rows.real * rows.real + rows.imag * rows.imag)[5:10]
    assert np.array_equal(bits(got[1]), bits((((p[0] + p[1]) + p[2]) + p[3]) + p[4]))
    assert ref.spectrum(x[: 64 * 7], h, 64, 4, 5).shape == (0, 64)


@pytest.mark.parametrize("K", [1, 5, 16, 17, 40])
def test_tone_lands_in_its_channel(oracle, K):
    """the prototype and tone of test_channelizer_tone_lands_in_its_channel: every integrated row has its maximum in the tone's channel"""
    h = oracle.lpf_corrected(1024, 0.45 / 64)
    k = 11
    n = np.arange(64 * 400)
    tone = np.exp(2j * np.pi * (k / 64) * n).astype(np.complex64)
    rows = ref.spectrum(tone, h, 64, 16, K)
    assert rows.shape == ((400 - 15) // K, 64)
    assert (rows.argmax(axis=1) == k).all()


@pytest.fixture(scope="module")
def emu_pfbspec():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_pspec"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pfb_pspec.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    E.emu_pfbspec.argtypes = [c64, C.c_long, C.c_long, C.c_int, C.c_long, C.c_long, f32, i32]
    E.emu_pfbspec.restype = C.c_long
    return E


@pytest.mark.parametrize("P", [4, 16])
@pytest.mark.parametrize("K", [1, 5, 16, 17, 40])
def test_fused_lane_programs(emu_pfbspec, oracle, P, K):
    """The sixty-four lane programs behind the transform, a wave per run of output rows and a wave per run of segments (and the fold
    thread program): with the launcher's own run length (at least three waves, the last one shorter) and with runs of 1 and 3 units,
    which end inside a tile -- bit for bit against the restatement, every output (or partial) element written exactly once."""
    M = 64
    least = -(-64 // K)
    nrows = 3 * least + 1
    h = oracle.synth_f32(9, P, M * P)
    x = oracle.synth_iq(SEED + K, 0, M * (nrows * K + P - 1) + M * (K - 1) + 5)  # a trailing partial row, and a few samples more
    assert ref.nrows(len(x), M, P, K) == nrows
    crows = ref.channel_rows(x, h, M, P, K)
    want = ref.spectrum(x, h, M, P, K)
    assert crows.shape == (nrows * K, M) and want.shape == (nrows, M)
    for upw, waves in ((0, 4), (1, nrows), (3, -(-nrows // 3))):
        out = np.full((nrows, M), np.nan, np.float32)
        stores = np.zeros(nrows * M, np.int32)
        assert emu_pfbspec.emu_pfbspec(crows, len(crows), K, 0, nrows, upw, out.reshape(-1), stores) == waves
        assert (stores == 1).all(), upw
        assert np.array_equal(bits(out), bits(want)), upw
    S = -(-K // pspec_ref.SEG)
    for upw in (0, 1, 3):
        part = np.full((nrows * S, M), np.nan, np.float32)
        stores = np.zeros(nrows * S * M, np.int32)
        nw = emu_pfbspec.emu_pfbspec(crows, len(crows), K, 1, nrows * S, upw, part.reshape(-1), stores)
        assert nw == -(-nrows * S // (upw or 4))  # the launcher's choice: four 16-row segments
        assert (stores == 1).all(), upw
        folded = part.reshape(nrows, S, M)[:, 0].copy()
        for s in range(1, S):
            folded = folded + part.reshape(nrows, S, M)[:, s]  # pspec_fold_thread's order
        assert np.array_equal(bits(folded), bits(want)), upw


NAMES = ["redio_pfb_pspec_" + n for n in ("create", "destroy", "nrows", "is_fused", "reserve", "enqueue", "enqueue_u8", "reserve_u8", "set_split")] + [
    f"redio_pfb_pspec_stream_{s}" for s in ("create", "create_u8", "destroy", "reset", "nout", "pending", "enqueue")]


def test_abi(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_pfb_pspec redio_pfb_pspec;" in hdr and "typedef struct redio_pfb_pspec_stream redio_pfb_pspec_stream;" in hdr
    for n in NAMES:
        assert hasattr(L, n), f"libredio.so does not export {n}"
        assert n + "(" in hdr
    R = redio.lib()
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    assert R.redio_pfb_pspec_create(None, taps, 64, 16, 4, 0) == -1
    assert R.redio_pfb_pspec_create(C.byref(p), taps, 64, 16, 0, 0) == -1
    assert R.redio_pfb_pspec_create(C.byref(p), None, 64, 16, 4, 0) == -1 and R.redio_pfb_pspec_create(C.byref(p), taps, 0, 16, 4, 0) == -1
    assert R.redio_pfb_pspec_create(C.byref(p), taps, 64, 0, 4, 0) == -1
    assert not p.value
    assert R.redio_pfb_pspec_nrows(None, 1 << 20) == 0 and R.redio_pfb_pspec_is_fused(None) == 0
    assert R.redio_pfb_pspec_destroy(None) == 0
    assert R.redio_pfb_pspec_reserve(None, 4096) == -1 and R.redio_pfb_pspec_reserve_u8(None, 4096) == -1
    assert R.redio_pfb_pspec_set_split(None, 1) == -1
    assert R.redio_pfb_pspec_enqueue(None, None, 4096, None, None) == -1 and R.redio_pfb_pspec_enqueue_u8(None, None, 4096, None, None) == -1
    assert R.redio_pfb_pspec_stream_create(C.byref(p), None) == -1 and R.redio_pfb_pspec_stream_create(None, None) == -1
    assert R.redio_pfb_pspec_stream_create_u8(C.byref(p), None) == -1
    assert R.redio_pfb_pspec_stream_nout(None, 5) == 0 and R.redio_pfb_pspec_stream_pending(None) == 0
    assert R.redio_pfb_pspec_stream_reset(None) == -1 and R.redio_pfb_pspec_stream_destroy(None) == 0
    assert R.redio_pfb_pspec_stream_enqueue(None, None, 5, None, None, None) == -1


def test_no_device_no_fallback(redio):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    assert redio.lib().redio_pfb_pspec_create(C.byref(p), taps, 64, 16, 4, 0) == -4 and not p.value
    with pytest.raises(redio.RedioError):
        redio.PolyphaseSpectrum(np.ones(1024, np.float32), 64, 16, 4)
