"""redio_pfb_os_synth_create / _enqueue refuse every bad argument before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import pfb_os_synth_ref as ref

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_create_refusals_and_null_handles(gpu, redio):
    L = redio.lib()
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    f = L.redio_pfb_os_synth_create
    assert f(None, taps, 64, 16, 32, 0) == ERR_ARG
    assert f(C.byref(p), None, 64, 16, 32, 0) == ERR_ARG and not p.value
    assert f(C.byref(p), taps, 0, 16, 1, 0) == ERR_ARG and not p.value
    assert f(C.byref(p), taps, 64, 0, 32, 0) == ERR_ARG and not p.value
    assert f(C.byref(p), taps, 64, -16, 32, 0) == ERR_ARG and not p.value
    assert f(C.byref(p), taps, 64, 16, 0, 0) == ERR_ARG and not p.value   # hop == 0
    assert f(C.byref(p), taps, 64, 16, 65, 0) == ERR_ARG and not p.value  # hop > nchan
    assert f(C.byref(p), taps, (1 << 26) + 1, 1, 1, 0) == ERR_UNSUPPORTED and not p.value  # redio_fft_create's
    assert L.redio_pfb_os_synth_route(None) == 0 and L.redio_pfb_os_synth_is_fused(None) == 0 and L.redio_pfb_os_synth_nout(None, 1 << 20) == 0
    assert L.redio_pfb_os_synth_hop(None) == 0
    assert L.redio_pfb_os_synth_set_unfused(None, 1) == ERR_ARG and L.redio_pfb_os_synth_reserve(None, 64) == ERR_ARG
    assert L.redio_pfb_os_synth_set_chunk_rows(None, 5) == ERR_ARG
    assert L.redio_pfb_os_synth_destroy(None) == OK
    s = C.c_void_p()
    assert L.redio_pfb_os_synth_stream_create(C.byref(s), None) == ERR_ARG and not s.value
    assert L.redio_pfb_os_synth_stream_create(None, None) == ERR_ARG
    assert L.redio_pfb_os_synth_stream_nout(None, 64) == 0 and L.redio_pfb_os_synth_stream_pending(None) == 0
    assert L.redio_pfb_os_synth_stream_reset(None) == ERR_ARG and L.redio_pfb_os_synth_stream_destroy(None) == OK


@pytest.mark.parametrize("M,P,H,unfused", [(64, 16, 32, False), (64, 4, 32, True), (128, 4, 32, False), (64, 4, 64, False)])
def test_misuse(gpu, redio, oracle, M, P, H, unfused):
    L = redio.lib()
    h = oracle.synth_f32(9, 0, M * P)
    plan = redio.OversampledSynthesizer(h, M, P, H)
    if unfused:
        plan.set_unfused(True)
    Lr = ref.nrows_per_hop(M, P, H)
    n = (Lr + 1) * M  # two hops
    X = oracle.synth_iq(7, 0, n + 2)
    dx = gpu.from_numpy(X).cuda()
    out = gpu.full((2 * H + 2,), 7.0, dtype=gpu.complex64, device="cuda")
    st = redio.current_stream()
    px, po = dx.data_ptr(), out.data_ptr()
    assert px % 16 == 0 and po % 16 == 0
    vp = C.c_void_p
    f = L.redio_pfb_os_synth_enqueue
    assert f(None, vp(px), n, 0, vp(po), st) == ERR_ARG
    assert f(plan._h, None, n, 0, vp(po), st) == ERR_ARG and f(plan._h, vp(px), n, 0, None, st) == ERR_ARG
    assert f(plan._h, vp(px + 4), n, 0, vp(po), st) == ERR_ARG                  # d_rows on a 4-byte boundary
    assert f(plan._h, vp(px), n, 0, vp(po + 4), st) == ERR_ARG                  # d_out on a 4-byte boundary
    assert f(plan._h, vp(po), n, 0, vp(po), st) == ERR_ARG                      # in place
    assert f(plan._h, vp(px), n, 0, vp(px + 8 * n - 8), st) == ERR_ARG          # the output starts on the last value read
    assert f(plan._h, vp(px + 8 * (2 * H - 1)), n, 0, vp(px), st) == ERR_ARG    # the input starts on the last sample written
    assert f(plan._h, vp(px), Lr * M - 1, 0, vp(po), st) == OK                  # fewer than L rows: nothing to do
    assert f(plan._h, None, Lr * M - 1, 0, None, st) == OK
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and np.array_equal(bits(dx.cpu().numpy()), bits(X))  # nothing was launched
    assert f(plan._h, vp(px + 8), n, 3, vp(po + 8), st) == OK                   # a whole-value boundary is enough
    gpu.cuda.synchronize()
    want = ref.synth(X[1: 1 + n], h, M, P, H, 3, True)
    o = out.cpu().numpy()
    assert np.array_equal(bits(o[1: 1 + 2 * H]), bits(want)) and o[0] == 7.0 and o[-1] == 7.0


def test_stream_refuses_a_misaligned_message_before_it_launches(gpu, redio, oracle):
    M, P, H = 64, 4, 32
    W = ref.nrows_per_hop(M, P, H) * M
    h = oracle.synth_f32(9, 0, M * P)
    X = oracle.synth_iq(7, 1, 3 * W)
    dx = gpu.from_numpy(X).cuda()
    plan = redio.OversampledSynthesizer(h, M, P, H)
    s = redio.OversampledSynthesizerStream(plan)
    assert s(dx[:10]).numel() == 0 and s.pending == 10
    out = gpu.full((8 * W,), 7.0, dtype=gpu.complex64, device="cuda")
    got = C.c_size_t(99)
    fn = redio.lib().redio_pfb_os_synth_stream_enqueue
    for nval in (5, 2 * W):
        assert fn(s._h, C.c_void_p(dx.data_ptr() + 84), nval, C.c_void_p(out.data_ptr()), C.byref(got), redio.current_stream()) == ERR_ARG
        assert got.value == 0 and s.pending == 10
    assert fn(s._h, C.c_void_p(dx.data_ptr() + 80), 2 * W, None, C.byref(got), redio.current_stream()) == ERR_ARG and s.pending == 10
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())
    y = s(dx[10:])
    assert np.array_equal(bits(y.cpu().numpy()), bits(ref.synth(X, h, M, P, H, 0, True)))
