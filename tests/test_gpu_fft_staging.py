"""The sizes at which a complex transform goes through its plan's staging buffer (fft_route.h: a route that cannot run in place, or
one whose generic-radix stages need a work buffer), on the plan itself and inside the plans that own one: without a reserve a capture is
refused (REDIO_ERR_NOT_RESERVED) and the stream works on; after the reserve the captured call allocates nothing and replays the
oracle's bits.  The smallest size of each kind: 32768 (multi-pass), 49152 = 3 * 2^14 (tile passes), 8194 = 2 * 17 * 241 (global stages
with a work buffer)."""
import numpy as np
import pytest

import fftr_ref
import pspec_ref

pytestmark = pytest.mark.gpu

ERR_NOT_RESERVED = -6
SEED = 0x5EED57A6
BATCH = 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def replay_twice(gpu, g, refill, out, want):
    for _ in range(2):
        refill()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy().reshape(-1)), bits(want.reshape(-1)))


@pytest.mark.parametrize("n,in_place", [(32768, True), (49152, True), (8194, False)])
def test_fft_capture(gpu, redio, oracle, n, in_place):
    x = oracle.synth_iq(SEED + n, 0, BATCH * n)
    want = oracle.fft(x, n, False)
    xd = gpu.from_numpy(x).cuda()
    src = xd.clone()
    dst = src if in_place else gpu.zeros_like(xd)

    plan = redio.Fft(n)
    with pytest.raises(redio.RedioError) as e:
        with redio.Graph():
            plan(src, out=dst)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(plan(src, out=dst).cpu().numpy()), bits(want))  # the capture ended cleanly: the stream and the plan work on

    plan = redio.Fft(n)
    plan.reserve(BATCH)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(src, out=dst)

    def refill():
        src.copy_(xd)
        if not in_place:
            dst.zero_()

    replay_twice(gpu, g, refill, dst, want)
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("inverse", [False, True])
def test_fftr_capture(gpu, redio, oracle, inverse):
    """16388 real points: the complex plan has 8194"""
    N = 16388
    if inverse:
        x = oracle.synth_iq(SEED + 1, 0, BATCH * (N // 2 + 1))
        want = fftr_ref.fftri_rows(x, N)
    else:
        x = oracle.synth_f32(SEED + 2, 0, BATCH * N)
        want = fftr_ref.fftr_rows(x, N)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32 if inverse else gpu.complex64, device="cuda")
    plan = redio.Fftr(N, inverse)
    plan.reserve(BATCH)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(xd, out=out)
    replay_twice(gpu, g, out.zero_, out, want)
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("N,windowed", [(8194, False), (32768, True)])
def test_power_spectrum_capture(gpu, redio, oracle, N, windowed):
    """K = 2, step = N.  The window makes the plan gather its rows and run the transform in place on them: the multi-pass route at 32768"""
    K = 2
    w = oracle.lpf_corrected(N, 0.1) if windowed else None
    n = 2 * K * N  # two rows
    x = oracle.synth_iq(SEED + 3 + N, 0, n)
    want = pspec_ref.power_spectrum(x, N, K, N, w)
    assert want.shape == (2, N)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K, N, w)
    plan.reserve(n)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(xd, out=out)
    replay_twice(gpu, g, out.zero_, out, want)
    assert redio.lib().redio_malloc_count() == count
