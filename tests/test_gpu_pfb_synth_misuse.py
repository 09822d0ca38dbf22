"""redio_pfb_synth_create / _enqueue refuse every bad argument before anything is launched."""
import ctypes as C

import numpy as np
import pytest

import pfb_synth_ref as ref

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_create_refusals_and_null_handles(gpu, redio):
    L = redio.lib()
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    assert L.redio_pfb_synth_create(None, taps, 64, 16, 0) == ERR_ARG
    assert L.redio_pfb_synth_create(C.byref(p), None, 64, 16, 0) == ERR_ARG and not p.value
    assert L.redio_pfb_synth_create(C.byref(p), taps, 0, 16, 0) == ERR_ARG and not p.value    # redio_pfb_create's own refusals
    assert L.redio_pfb_synth_create(C.byref(p), taps, 64, 0, 0) == ERR_ARG and not p.value
    assert L.redio_pfb_synth_create(C.byref(p), taps, 64, -16, 0) == ERR_ARG and not p.value
    assert L.redio_pfb_synth_create(C.byref(p), taps, (1 << 26) + 1, 1, 0) == ERR_UNSUPPORTED and not p.value  # redio_fft_create's
    assert L.redio_pfb_synth_route(None) == 0 and L.redio_pfb_synth_is_fused(None) == 0 and L.redio_pfb_synth_nout(None, 1 << 20) == 0
    assert L.redio_pfb_synth_set_unfused(None, 1) == ERR_ARG and L.redio_pfb_synth_reserve(None, 64) == ERR_ARG
    assert L.redio_pfb_synth_destroy(None) == OK
    s = C.c_void_p()
    assert L.redio_pfb_synth_stream_create(C.byref(s), None) == ERR_ARG and not s.value
    assert L.redio_pfb_synth_stream_create(None, None) == ERR_ARG
    assert L.redio_pfb_synth_stream_nout(None, 64) == 0 and L.redio_pfb_synth_stream_pending(None) == 0
    assert L.redio_pfb_synth_stream_reset(None) == ERR_ARG and L.redio_pfb_synth_stream_destroy(None) == OK


@pytest.mark.parametrize("M,P,unfused", [(64, 16, False), (64, 4, True), (128, 4, False)])
def test_misuse(gpu, redio, oracle, M, P, unfused):
    L = redio.lib()
    h = oracle.synth_f32(9, 0, M * P)
    plan = redio.Synthesizer(h, M, P)
    if unfused:
        plan.set_unfused(True)
    n = M * (P + 1)  # two output rows
    x = oracle.synth_iq(7, 0, n + 2)
    dx = gpu.from_numpy(x).cuda()
    out = gpu.full((2 * M + 2,), 7.0, dtype=gpu.complex64, device="cuda")
    st = redio.current_stream()
    px, po = dx.data_ptr(), out.data_ptr()
    assert px % 16 == 0 and po % 16 == 0
    vp = C.c_void_p
    f = L.redio_pfb_synth_enqueue
    assert f(None, vp(px), n, vp(po), st) == ERR_ARG
    assert f(plan._h, None, n, vp(po), st) == ERR_ARG and f(plan._h, vp(px), n, None, st) == ERR_ARG
    assert f(plan._h, vp(px + 4), n, vp(po), st) == ERR_ARG                  # d_in on a 4-byte boundary
    assert f(plan._h, vp(px), n, vp(po + 4), st) == ERR_ARG                  # d_out on a 4-byte boundary
    assert f(plan._h, vp(po), n, vp(po), st) == ERR_ARG                      # in place
    assert f(plan._h, vp(px), n, vp(px + 8 * n - 8), st) == ERR_ARG          # the output starts on the last value read
    assert f(plan._h, vp(px + 8 * (2 * M - 1)), n, vp(px), st) == ERR_ARG    # the input starts on the last sample written
    assert f(plan._h, vp(px), P * M - 1, vp(po), st) == OK                   # fewer than P M values: nothing to do
    assert f(plan._h, None, P * M - 1, None, st) == OK
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and np.array_equal(bits(dx.cpu().numpy()), bits(x))  # nothing was launched
    assert f(plan._h, vp(px + 8), n, vp(po + 8), st) == OK                   # a whole-value boundary is enough
    gpu.cuda.synchronize()
    want = ref.synth(x[1: 1 + n], h, M, P, True)
    o = out.cpu().numpy()
    assert np.array_equal(bits(o[1: 1 + 2 * M]), bits(want)) and o[0] == 7.0 and o[-1] == 7.0


def test_stream_refuses_a_misaligned_message_before_it_launches(gpu, redio, oracle):
    M, P = 64, 4
    h = oracle.synth_f32(9, 0, M * P)
    x = oracle.synth_iq(7, 1, 3 * P * M)
    dx = gpu.from_numpy(x).cuda()
    plan = redio.Synthesizer(h, M, P)
    s = redio.SynthesizerStream(plan)
    assert s(dx[:10]).numel() == 0 and s.pending == 10
    out = gpu.full((4 * P * M,), 7.0, dtype=gpu.complex64, device="cuda")
    got = C.c_size_t(99)
    fn = redio.lib().redio_pfb_synth_stream_enqueue
    for nval in (5, 2 * P * M):
        assert fn(s._h, C.c_void_p(dx.data_ptr() + 84), nval, C.c_void_p(out.data_ptr()), C.byref(got), redio.current_stream()) == ERR_ARG
        assert got.value == 0 and s.pending == 10
    assert fn(s._h, C.c_void_p(dx.data_ptr() + 80), 2 * P * M, None, C.byref(got), redio.current_stream()) == ERR_ARG and s.pending == 10
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())
    y = s(dx[10:])
    assert np.array_equal(bits(y.cpu().numpy()), bits(ref.synth(x, h, M, P, True)))
