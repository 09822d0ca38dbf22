"""Every argument error of the tuned resampler's C ABI (include/redio.h, redio_ddc_upfirdn_*) returns its code, and nothing is launched:
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
    w = np.ascontiguousarray(oracle.synth_iq(1, 0, 24)).view(np.float32)
    big = np.zeros(2 * 65537, np.float32)
    taps = oracle.synth_f32(2, 0, 31)
    h = C.c_void_p()
    create = L.redio_ddc_upfirdn_create
    # the tuner's refusals
    assert create(None, fp(w), 24, fp(taps), 31, 3, 2, 0) == ARG
    assert create(C.byref(h), None, 24, fp(taps), 31, 3, 2, 0) == ARG and not h.value
    assert create(C.byref(h), fp(w), 24, None, 31, 3, 2, 0) == ARG and not h.value
    assert create(C.byref(h), fp(w), 0, fp(taps), 31, 3, 2, 0) == ARG and not h.value
    assert create(C.byref(h), fp(big), 65537, fp(taps), 31, 3, 2, 0) == ARG and not h.value
    assert create(C.byref(h), fp(w), 24, fp(taps), 0, 3, 2, 0) == ARG and not h.value
    # the resampler's
    assert create(C.byref(h), fp(w), 24, fp(taps), 31, 0, 2, 0) == ARG and not h.value
    assert create(C.byref(h), fp(w), 24, fp(taps), 31, 3, 0, 0) == ARG and not h.value
    assert create(C.byref(h), fp(w), 24, fp(taps), 2 ** 24 + 1, 3, 2, 0) == UNSUPPORTED and not h.value  # refused before the taps are read
    assert create(C.byref(h), fp(w), 24, fp(taps), 31, 65537, 2, 0) == UNSUPPORTED and not h.value
    assert create(C.byref(h), fp(w), 24, fp(taps), 31, 3, 2 ** 31, 0) == UNSUPPORTED and not h.value
    assert create(C.byref(h), fp(big), 65536, fp(taps), 31, 65536, 2, 0) == 0 and h.value  # the caps themselves are taken
    assert L.redio_ddc_upfirdn_period(h) == 65536 and L.redio_ddc_upfirdn_route(h) == 2
    assert L.redio_ddc_upfirdn_period_out(h) == 32768 and L.redio_ddc_upfirdn_period_in(h) == 1 and L.redio_ddc_upfirdn_window(h) == 2
    assert L.redio_ddc_upfirdn_nout(h, 10) == (10 * 65536 - 31) // 2 + 1 and L.redio_ddc_upfirdn_nout(h, 2 ** 46 + 1) == 0
    assert L.redio_ddc_upfirdn_destroy(h) == 0 and L.redio_ddc_upfirdn_destroy(None) == 0
    for name in ("period", "route", "period_out", "period_in", "window"):
        assert getattr(L, f"redio_ddc_upfirdn_{name}")(None) == 0
    assert L.redio_ddc_upfirdn_nout(None, 100) == 0
    s = C.c_void_p()
    assert L.redio_ddc_upfirdn_stream_create(C.byref(s), None) == ARG and not s.value
    assert L.redio_ddc_upfirdn_stream_create_u8(C.byref(s), None) == ARG and L.redio_ddc_upfirdn_stream_create(None, None) == ARG
    assert L.redio_ddc_upfirdn_stream_index(None) == 0 and L.redio_ddc_upfirdn_stream_reset(None) == ARG
    assert L.redio_ddc_upfirdn_stream_destroy(None) == 0
    assert L.redio_ddc_upfirdn_stream_nout(None, 10) == 0 and L.redio_ddc_upfirdn_stream_pending(None) == 0
    got = C.c_size_t(5)
    assert L.redio_ddc_upfirdn_stream_enqueue(None, None, 10, None, C.byref(got), None) == ARG


@pytest.mark.parametrize("U,D", [(3, 2), (3, 16)])  # both routes
def test_enqueue_refusals_launch_nothing(gpu, redio, oracle, U, D):
    L = redio.lib()
    plan = redio.DdcUpfirdn(oracle.synth_iq(1, 0, 24), oracle.synth_f32(2, 0, 31), U, D)
    assert plan.route == (1 if D == 2 else 2)
    st = redio.current_stream()
    xh = oracle.synth_iq(3, 0, 4096)
    x = gpu.from_numpy(xh).cuda()
    raw = gpu.from_numpy(np.arange(8192, dtype=np.uint8)).cuda()
    out = gpu.full((8192,), 7.0, dtype=gpu.complex64, device="cuda")
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    enq, enq8 = L.redio_ddc_upfirdn_enqueue, L.redio_ddc_upfirdn_enqueue_u8
    assert enq(None, p(x), 4096, 0, p(out), st) == ARG
    assert enq8(None, p(raw), 8192, 0, p(out), st) == ARG
    assert enq(plan._h, None, 4096, 0, p(out), st) == ARG
    assert enq(plan._h, p(x), 4096, 0, None, st) == ARG
    assert enq8(plan._h, None, 8192, 0, p(out), st) == ARG
    assert enq8(plan._h, p(raw), 8192, 0, None, st) == ARG
    assert enq8(plan._h, p(raw), 8191, 0, p(out), st) == ARG        # odd nbytes
    assert enq(plan._h, p(x), 4096, 0, p(x), st) == ARG              # in == out
    assert enq(plan._h, p(x), 4096, 0, p(x, 8 * 100), st) == ARG     # out inside in
    assert enq(plan._h, p(x, 8 * 100), 3000, 0, p(x), st) == ARG     # in inside out's range
    assert enq8(plan._h, p(raw), 8192, 0, p(raw, 64), st) == ARG     # out inside the bytes
    assert enq(plan._h, p(x, 4), 3000, 0, p(out), st) == ARG         # cf32 not on a whole sample
    assert enq(plan._h, p(x), 3000, 0, p(out, 4), st) == ARG
    assert enq8(plan._h, p(raw), 8192, 0, p(out, 4), st) == ARG
    assert plan.nout(31 // U) == 0
    assert enq(plan._h, p(x), 31 // U, 0, None, st) == 0             # no output is due: nothing to do
    assert enq8(plan._h, p(raw), 2 * (31 // U), 0, None, st) == 0
    gpu.cuda.synchronize()
    assert (out.cpu().numpy() == 7.0).all()
    assert (x.cpu().numpy() == xh).all() and (raw.cpu().numpy() == np.arange(8192, dtype=np.uint8)).all()
    # and bytes are taken at any alignment: the call itself goes through
    assert enq8(plan._h, p(raw, 1), 8190, 0, p(out), st) == 0
    gpu.cuda.synchronize()
