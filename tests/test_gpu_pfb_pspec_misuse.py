"""redio_pfb_pspec_enqueue / _enqueue_u8 refuse every bad argument before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, -1


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_create_refusals(gpu, redio, oracle):
    L = redio.lib()
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    assert L.redio_pfb_pspec_create(C.byref(p), taps, 64, 16, 0, 0) == ERR_ARG and not p.value        # integrate == 0
    assert L.redio_pfb_pspec_create(C.byref(p), taps, 0, 16, 4, 0) == ERR_ARG and not p.value         # redio_pfb_create's own
    assert L.redio_pfb_pspec_create(C.byref(p), None, 64, 16, 4, 0) == ERR_ARG and not p.value
    assert L.redio_pfb_pspec_create(C.byref(p), taps, 64, -16, 4, 0) == ERR_ARG and not p.value
    plan = redio.PolyphaseSpectrum(np.ones(256, np.float32), 64, 4, 3)
    assert L.redio_pfb_pspec_set_split(plan._h, 3) == ERR_ARG and L.redio_pfb_pspec_set_split(plan._h, -1) == ERR_ARG


@pytest.mark.parametrize("M,P,K", [(64, 16, 4), (128, 4, 3)])
def test_misuse(gpu, redio, oracle, M, P, K):
    L = redio.lib()
    h = oracle.synth_f32(9, 0, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    n = M * (2 * K + P - 1)  # two rows
    raw = np.random.default_rng(M).integers(0, 256, 2 * n + 16, dtype=np.uint8)
    x = oracle.synth_iq(7, 0, n + 2)
    big, dx = gpu.from_numpy(raw).cuda(), gpu.from_numpy(x).cuda()
    out = gpu.full((2 * M + 2,), 7.0, dtype=gpu.float32, device="cuda")
    st = redio.current_stream()
    pb, px, po = big.data_ptr(), dx.data_ptr(), out.data_ptr()
    assert pb % 8 == 0 and px % 8 == 0 and po % 8 == 0
    vp = C.c_void_p
    f8, fc = L.redio_pfb_pspec_enqueue_u8, L.redio_pfb_pspec_enqueue
    assert f8(plan._h, vp(pb), 2 * n - 1, vp(po), st) == ERR_ARG          # odd nbytes
    assert f8(plan._h, vp(pb + 1), 2 * n, vp(po), st) == ERR_ARG          # d_bytes at an odd address
    assert f8(plan._h, vp(pb), 2 * n, vp(po + 2), st) == ERR_ARG          # d_out on a 2-byte boundary
    assert f8(plan._h, None, 2 * n, vp(po), st) == ERR_ARG and f8(plan._h, vp(pb), 2 * n, None, st) == ERR_ARG
    assert f8(None, vp(pb), 2 * n, vp(po), st) == ERR_ARG
    assert f8(plan._h, vp(po + 4), 2 * n, vp(po), st) == ERR_ARG          # the bytes lie inside the output range
    assert f8(plan._h, vp(pb), 2 * n, vp(pb + 2 * n - 8), st) == ERR_ARG  # the output starts on the last four samples
    assert fc(plan._h, vp(px + 4), n, vp(po), st) == ERR_ARG              # d_in on a 4-byte boundary
    assert fc(plan._h, vp(px), n, vp(po + 2), st) == ERR_ARG
    assert fc(plan._h, None, n, vp(po), st) == ERR_ARG and fc(plan._h, vp(px), n, None, st) == ERR_ARG
    assert fc(None, vp(px), n, vp(po), st) == ERR_ARG
    assert fc(plan._h, vp(px), n, vp(px + 8 * n - 8), st) == ERR_ARG      # the output starts on the last sample
    assert fc(plan._h, vp(po), n, vp(po), st) == ERR_ARG                  # in place
    short = M * (K + P - 1) - 1
    assert fc(plan._h, vp(px), short, vp(po), st) == OK and f8(plan._h, vp(pb), 2 * short, vp(po), st) == OK  # too few samples: nothing to do
    assert fc(plan._h, None, short, None, st) == OK
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and np.array_equal(big.cpu().numpy(), raw) and np.array_equal(bits(dx.cpu().numpy()), bits(x))  # nothing was launched
    assert f8(plan._h, vp(pb + 2), 2 * n, vp(po), st) == OK                # a whole-sample boundary is enough
    gpu.cuda.synchronize()
    want = ref.spectrum_u8(raw[2: 2 + 2 * n], h, M, P, K, True)
    assert np.array_equal(bits(out[: 2 * M].cpu().numpy()), bits(want.reshape(-1))) and bool((out[2 * M:] == 7.0).all())
    assert fc(plan._h, vp(px + 8), n, vp(po), st) == OK
    gpu.cuda.synchronize()
    want = ref.spectrum(x[1: 1 + n], h, M, P, K, True)
    assert np.array_equal(bits(out[: 2 * M].cpu().numpy()), bits(want.reshape(-1))) and bool((out[2 * M:] == 7.0).all())


def test_u8_stream_refuses_an_odd_address_before_it_launches(gpu, redio, oracle):
    M, P, K = 64, 4, 3
    W = (K - 1 + P) * M
    h = oracle.synth_f32(9, 0, M * P)
    raw = np.random.default_rng(3).integers(0, 256, 2 * (3 * W) + 2, dtype=np.uint8)
    big = gpu.from_numpy(raw).cuda()
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    s = redio.Stream(plan, u8=True)
    first = s(big[: 2 * 10])
    assert first.numel() == 0 and s.pending == 10
    out = gpu.full((4 * M,), 7.0, dtype=gpu.float32, device="cuda")
    got = C.c_size_t(99)
    fn = redio.lib().redio_pfb_pspec_stream_enqueue
    for nsamp in (5, 2 * W):
        assert fn(s._h, C.c_void_p(big.data_ptr() + 21), nsamp, C.c_void_p(out.data_ptr()), C.byref(got), redio.current_stream()) == ERR_ARG
        assert got.value == 0 and s.pending == 10
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())
    y = s(big[20: 2 * (3 * W)])
    want = ref.spectrum_u8(raw[: 2 * (3 * W)], h, M, P, K, True)
    assert np.array_equal(bits(y.cpu().numpy()), bits(want.reshape(-1)))
