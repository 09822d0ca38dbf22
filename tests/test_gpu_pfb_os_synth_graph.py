"""The oversampled synthesis bank under stream capture: the wave kernel captures and replays without a reserve, the two-pass route
un-reserved refuses to allocate inside a capture and launches nothing, and after reserve it captures; no enqueue allocates."""
import numpy as np
import pytest

import pfb_os_synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0536
ERR_NOT_RESERVED = -6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu, oracle, M, P, H, hops):
    h = oracle.synth_f32(9, 0, M * P)
    X = oracle.synth_iq(SEED, M, (hops + ref.nrows_per_hop(M, P, H) - 1) * M + 3)
    want = ref.synth(X, h, M, P, H, 1, True)
    return h, gpu.from_numpy(X).cuda(), want, gpu.full((want.size,), 7.0, dtype=gpu.complex64, device="cuda")


@pytest.mark.parametrize("P", [4, 16])
def test_wave_kernel_captures_without_a_reserve(gpu, redio, oracle, P):
    h, d, want, out = make(gpu, oracle, 64, P, 32, 150)
    plan = redio.OversampledSynthesizer(h, 64, P, 32)
    assert plan.route == 1
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, first_row=1, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("M,P,H,unfused", [(128, 8, 64, False), (64, 16, 32, True), (12, 2, 5, False)])
def test_two_pass_needs_the_reserve_and_then_captures(gpu, redio, oracle, M, P, H, unfused):
    h, d, want, out = make(gpu, oracle, M, P, H, 50)
    plan = redio.OversampledSynthesizer(h, M, P, H)
    if unfused:
        plan.set_unfused(True)
    assert plan.route == 0
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(d, first_row=1, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
    plan.reserve(d.numel())
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, first_row=1, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert np.array_equal(bits(plan(d, first_row=1, out=out).cpu().numpy()), bits(want))  # and un-captured, on the same scratch
    assert redio.lib().redio_malloc_count() == count  # reserved: no enqueue allocated
