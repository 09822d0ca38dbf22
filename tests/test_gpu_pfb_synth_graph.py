"""The synthesis filterbank under stream capture: the wave kernel captures and replays without a reserve, the two-pass route
un-reserved refuses to allocate inside a capture and launches nothing, and after reserve it captures; no enqueue allocates."""
import numpy as np
import pytest

import pfb_synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED5179
ERR_NOT_RESERVED = -6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu, oracle, M, P, rows):
    h = oracle.synth_f32(9, 0, M * P)
    x = oracle.synth_iq(SEED, M, (rows + P - 1) * M + 3)
    want = ref.synth(x, h, M, P, True)
    return h, gpu.from_numpy(x).cuda(), want, gpu.full((len(want),), 7.0, dtype=gpu.complex64, device="cuda")


@pytest.mark.parametrize("P", [4, 16])
def test_wave_kernel_captures_without_a_reserve(gpu, redio, oracle, P):
    h, d, want, out = make(gpu, oracle, 64, P, 150)
    plan = redio.Synthesizer(h, 64, P)
    assert plan.route == 1
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("M,P,unfused", [(128, 8, False), (64, 16, True), (12, 3, False)])
def test_two_pass_needs_the_reserve_and_then_captures(gpu, redio, oracle, M, P, unfused):
    h, d, want, out = make(gpu, oracle, M, P, 50)
    plan = redio.Synthesizer(h, M, P)
    if unfused:
        plan.set_unfused(True)
    assert plan.route == 0
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(d, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    plan.reserve(d.numel())
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert np.array_equal(bits(plan(d, out=out).cpu().numpy()), bits(want))  # and un-captured, on the same scratch
    assert redio.lib().redio_malloc_count() == count  # reserved: no enqueue allocated


def test_a_plan_finalised_inside_a_capture_waits_for_its_end(gpu, redio, oracle):
    """A plan left in a reference cycle (what `pytest.raises(...) as e` does to a test's locals) is finalised wherever the collector
    next runs.  Inside a Graph capture on the same thread its destroy, which frees device memory, would invalidate the capture: it
    waits for the capture's end, the capture replays, and the plan is destroyed then."""
    import gc
    from libredio_amd import plans
    h, d, want, out = make(gpu, oracle, 64, 4, 40)
    plan = redio.Synthesizer(h, 64, 4)
    gc.collect()
    gc.disable()  # the collector runs where this test says
    try:
        dead = redio.Synthesizer(oracle.synth_f32(9, 0, 36), 12, 3)
        dead.reserve(12 * 20)  # route 0: it owns scratch
        dead.me = dead
        del dead
        g = redio.Graph()
        with g:
            assert gc.collect() >= 1 and len(plans._deferred) == 1
            plan(d, out=out)
        assert plans._deferred == []
    finally:
        gc.enable()
    out.zero_()
    g.launch()
    gpu.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
