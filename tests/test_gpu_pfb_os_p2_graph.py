"""The oversampled channelizer's workgroup kernel (route 2) under stream capture: it captures WITHOUT a reserve and replays on fresh
input, no enqueue allocates; the same plan sent down route 0 un-reserved still refuses to allocate inside a capture."""
import numpy as np
import pytest

import pfb_os_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0B53
ERR_NOT_RESERVED = -6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("M,P", [(128, 8), (1024, 4)])
def test_route_2_captures_without_a_reserve(gpu, redio, oracle, M, P):
    H, rows = M // 2, 70
    n = M * P + (rows - 1) * H + 3
    h = oracle.synth_f32(9, 0, M * P)
    xs = [oracle.synth_iq(SEED + i, M, n) for i in range(2)]
    wants = [ref.channelize(x, h, M, P, H, 1, True) for x in xs]
    d = gpu.zeros(n, dtype=gpu.complex64, device="cuda")
    out = gpu.full((rows * M,), 7.0, dtype=gpu.complex64, device="cuda")
    plan = redio.OversampledChannelizer(h, M, P, H, one_kernel=True)
    assert plan.route == 2
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, first_row=1, out=out)
    for x, want in zip(xs, wants):  # replayed twice, each time on fresh input
        d.copy_(gpu.from_numpy(x))
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count


def test_the_same_plan_unfused_still_needs_the_reserve(gpu, redio, oracle):
    M, P, H, rows = 128, 8, 64, 50
    h = oracle.synth_f32(9, 0, M * P)
    x = oracle.synth_iq(SEED, M, M * P + (rows - 1) * H)
    d = gpu.from_numpy(x).cuda()
    out = gpu.full((rows * M,), 7.0, dtype=gpu.complex64, device="cuda")
    plan = redio.OversampledChannelizer(h, M, P, H, one_kernel=True)
    plan.set_unfused(True)
    assert plan.route == 0
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(d, first_row=1, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())  # nothing was launched
