"""Every argument error of the rational resampler's C ABI (include/redio.h, redio_upfirdn_*) returns its code, and nothing is launched:
the output buffer keeps its bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = -1, -3  # REDIO_ERR_ARG, REDIO_ERR_UNSUPPORTED
_pf = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(_pf)


def test_create_refusals(gpu, redio, oracle):
    L = redio.lib()
    taps = oracle.synth_f32(2, 0, 31)
    h = C.c_void_p()
    assert L.redio_upfirdn_create(None, fp(taps), 31, 3, 2, 0) == ARG
    assert L.redio_upfirdn_create(C.byref(h), None, 31, 3, 2, 0) == ARG and not h.value
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 0, 3, 2, 0) == ARG and not h.value
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 31, 0, 2, 0) == ARG and not h.value
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 31, 3, 0, 0) == ARG and not h.value
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 2 ** 24 + 1, 3, 2, 0) == UNSUPPORTED and not h.value  # refused before the taps are read
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 31, 65537, 2, 0) == UNSUPPORTED and not h.value
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 31, 3, 2 ** 31, 0) == UNSUPPORTED and not h.value
    assert L.redio_upfirdn_create(C.byref(h), fp(taps), 31, 65536, 2, 0) == 0 and h.value  # the cap itself is taken
    assert L.redio_upfirdn_period_out(h) == 32768 and L.redio_upfirdn_period_in(h) == 1 and L.redio_upfirdn_route(h) == 2
    assert L.redio_upfirdn_window(h) == 2 and L.redio_upfirdn_nout(h, 10) == (10 * 65536 - 31) // 2 + 1
    assert L.redio_upfirdn_destroy(h) == 0 and L.redio_upfirdn_destroy(None) == 0
    assert L.redio_upfirdn_nout(None, 100) == 0 and L.redio_upfirdn_route(None) == 0
    assert L.redio_upfirdn_period_out(None) == 0 and L.redio_upfirdn_period_in(None) == 0 and L.redio_upfirdn_window(None) == 0
    s = C.c_void_p()
    assert L.redio_upfirdn_stream_create(C.byref(s), None) == ARG and not s.value
    assert L.redio_upfirdn_stream_create(None, None) == ARG
    assert L.redio_upfirdn_stream_reset(None) == ARG and L.redio_upfirdn_stream_destroy(None) == 0
    assert L.redio_upfirdn_stream_nout(None, 10) == 0 and L.redio_upfirdn_stream_pending(None) == 0
    got = C.c_size_t(5)
    assert L.redio_upfirdn_stream_enqueue(None, None, 10, None, C.byref(got), None) == ARG


@pytest.mark.parametrize("U,D", [(3, 2), (3, 16)])  # both routes
def test_enqueue_refusals_launch_nothing(gpu, redio, oracle, U, D):
    L = redio.lib()
    plan = redio.Upfirdn(oracle.synth_f32(2, 0, 31), U, D, complex_input=True)
    st = redio.current_stream()
    x = gpu.from_numpy(oracle.synth_iq(3, 0, 4096)).cuda()
    out = gpu.full((8192,), 7.0, dtype=gpu.complex64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert L.redio_upfirdn_enqueue(None, p(x), 4096, p(out), st) == ARG
    assert L.redio_upfirdn_enqueue(plan._h, None, 4096, p(out), st) == ARG
    assert L.redio_upfirdn_enqueue(plan._h, p(x), 4096, None, st) == ARG
    assert L.redio_upfirdn_enqueue(plan._h, p(x), 4096, p(x), st) == ARG            # in == out
    assert L.redio_upfirdn_enqueue(plan._h, p(x), 4096, p(x, 8 * 100), st) == ARG   # out inside in
    assert L.redio_upfirdn_enqueue(plan._h, p(x, 8 * 100), 3000, p(x), st) == ARG   # in inside out's range
    assert L.redio_upfirdn_enqueue(plan._h, p(x, 4), 3000, p(out), st) == ARG       # not on a whole sample
    assert L.redio_upfirdn_enqueue(plan._h, p(x), 3000, p(out, 4), st) == ARG
    assert plan.nout(31 // U) == 0
    assert L.redio_upfirdn_enqueue(plan._h, p(x), 31 // U, None, st) == 0           # no output is due: nothing to do
    gpu.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    assert (x.cpu().numpy() == oracle.synth_iq(3, 0, 4096)).all()
