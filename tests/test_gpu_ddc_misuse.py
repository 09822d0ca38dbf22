"""Every argument error of the tuner's C ABI (include/redio.h, redio_ddc_*) returns its code, and nothing is launched: the output buffer
keeps its bytes."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARG = -1
_pf = C.POINTER(C.c_float)


def fp(a):
    return a.ctypes.data_as(_pf)


def test_create_refusals(gpu, redio, oracle):
    L = redio.lib()
    w = np.ascontiguousarray(oracle.synth_iq(1, 0, 24)).view(np.float32)
    big = np.zeros(2 * 65537, np.float32)
    taps = oracle.synth_f32(2, 0, 31)
    h = C.c_void_p()
    assert L.redio_ddc_create(None, fp(w), 24, fp(taps), 31, 2, 0) == ARG
    assert L.redio_ddc_create(C.byref(h), None, 24, fp(taps), 31, 2, 0) == ARG and not h.value
    assert L.redio_ddc_create(C.byref(h), fp(w), 24, None, 31, 2, 0) == ARG and not h.value
    assert L.redio_ddc_create(C.byref(h), fp(w), 0, fp(taps), 31, 2, 0) == ARG and not h.value
    assert L.redio_ddc_create(C.byref(h), fp(big), 65537, fp(taps), 31, 2, 0) == ARG and not h.value
    assert L.redio_ddc_create(C.byref(h), fp(w), 24, fp(taps), 0, 2, 0) == ARG and not h.value
    assert L.redio_ddc_create(C.byref(h), fp(w), 24, fp(taps), 31, 0, 0) == ARG and not h.value
    assert L.redio_ddc_create(C.byref(h), fp(big), 65536, fp(taps), 31, 2, 0) == 0 and h.value  # the cap itself is taken
    assert L.redio_ddc_period(h) == 65536 and L.redio_ddc_route(h) == 2
    assert L.redio_ddc_destroy(h) == 0 and L.redio_ddc_destroy(None) == 0
    assert L.redio_ddc_nout(None, 100) == 0 and L.redio_ddc_period(None) == 0 and L.redio_ddc_route(None) == 0
    s = C.c_void_p()
    assert L.redio_ddc_stream_create(C.byref(s), None) == ARG and not s.value
    assert L.redio_ddc_stream_create_u8(C.byref(s), None) == ARG and L.redio_ddc_stream_create(None, None) == ARG
    assert L.redio_ddc_stream_index(None) == 0 and L.redio_ddc_stream_reset(None) == ARG and L.redio_ddc_stream_destroy(None) == 0


def test_enqueue_refusals_launch_nothing(gpu, redio, oracle):
    L = redio.lib()
    plan = redio.Ddc(oracle.synth_iq(1, 0, 24), oracle.synth_f32(2, 0, 31), 2)
    st = redio.current_stream()
    x = gpu.from_numpy(oracle.synth_iq(3, 0, 4096)).cuda()
    raw = gpu.from_numpy(np.arange(8192, dtype=np.uint8)).cuda()
    out = gpu.full((4096,), 7.0, dtype=gpu.complex64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    assert L.redio_ddc_enqueue(None, p(x), 4096, 0, p(out), st) == ARG
    assert L.redio_ddc_enqueue_u8(None, p(raw), 8192, 0, p(out), st) == ARG
    assert L.redio_ddc_enqueue(plan._h, None, 4096, 0, p(out), st) == ARG
    assert L.redio_ddc_enqueue(plan._h, p(x), 4096, 0, None, st) == ARG
    assert L.redio_ddc_enqueue_u8(plan._h, p(raw), 8191, 0, p(out), st) == ARG   # odd nbytes
    assert L.redio_ddc_enqueue(plan._h, p(x), 4096, 0, p(x), st) == ARG           # in == out
    assert L.redio_ddc_enqueue(plan._h, p(x), 4096, 0, p(x, 8 * 100), st) == ARG  # out inside in
    assert L.redio_ddc_enqueue(plan._h, p(x, 8 * 100), 3000, 0, p(x), st) == ARG  # in inside out's range
    assert L.redio_ddc_enqueue_u8(plan._h, p(raw), 8192, 0, p(raw, 64), st) == ARG
    assert L.redio_ddc_enqueue(plan._h, p(x), 30, 0, None, st) == 0               # fewer than ntaps samples: nothing to do
    gpu.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    assert (x.cpu().numpy() == oracle.synth_iq(3, 0, 4096)).all()
