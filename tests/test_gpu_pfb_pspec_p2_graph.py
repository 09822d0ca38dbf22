"""The polyphase spectrometer's workgroup kernel (route 2) under stream capture and as a stream: a call by rows, or with K <= 16,
needs no scratch and captures without a reserve; a call by segments that finds its partials un-reserved refuses inside a capture and
works afterwards; after reserve it replays with equal bits and allocates nothing.  Then plans.Stream over a flagged plan, fed in
uneven pieces and again after reset(), from cf32 samples and from u8 I/Q bytes, against the restatement of the whole stream."""
import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F62
ERR_NOT_RESERVED = -6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(gpu, oracle, M, P, K, rows, u8):
    """(taps, device input, the restatement's rows, samples)"""
    h = oracle.synth_f32(9, 0, M * P)
    n = M * (rows * K + P - 1) + 3
    if u8:
        raw = np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8)
        return h, gpu.from_numpy(raw).cuda(), ref.spectrum_u8(raw, h, M, P, K, True), n
    x = oracle.synth_iq(SEED, 0, n)
    return h, gpu.from_numpy(x).cuda(), ref.spectrum(x, h, M, P, K, True), n


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("M,P,K,mode", [(128, 8, 5, 0), (128, 8, 5, 2), (128, 8, 17, 1), (1024, 4, 40, 1)])
def test_captures_without_a_reserve(gpu, redio, oracle, M, P, K, mode, u8):
    h, d, want, n = make(gpu, oracle, M, P, K, 5, u8)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK
    plan.set_split(mode)
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        (plan.from_bytes if u8 else plan)(d, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("M,P", [(128, 8), (512, 16)])
def test_segments_need_the_reserve(gpu, redio, oracle, M, P, u8):
    K = 17
    h, d, want, n = make(gpu, oracle, M, P, K, 5, u8)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK
    plan.set_split(plan.SEGMENTS)
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    run = plan.from_bytes if u8 else plan
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            run(d, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(run(d, out=out).cpu().numpy()), bits(want))  # the plan and the stream work on afterwards
    fresh = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    fresh.set_split(fresh.SEGMENTS)
    count = redio.lib().redio_malloc_count()
    fresh.reserve(n, u8=u8)
    assert redio.lib().redio_malloc_count() == count + 1  # the segment partials: no row scratch, no inner-channelizer scratch
    g = redio.Graph()
    with g:
        (fresh.from_bytes if u8 else fresh)(d, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count + 1


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("K", [5, 17])
def test_stream_gives_the_one_shot_bits(gpu, redio, oracle, K, u8):
    """256 x 8: messages of 1 sample, an odd count, less than a row, a window less a few, whole hops and several windows.  The carried
    tail puts a call's first sample at any offset, so the calls arrive at bases of either alignment."""
    M, P = 256, 8
    W, H = ref.shape(M, P, K)
    lens = [1, 7, M - 3, W - 9, 1, H, W, W + 1, 3 * H + 5, 333, 2 * W + H - 1, 1, H - 1]
    h = oracle.synth_f32(9, 0, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK
    if u8:
        raw = np.random.default_rng(SEED).integers(0, 256, 2 * sum(lens), dtype=np.uint8)
        d, want = gpu.from_numpy(raw).cuda(), ref.spectrum_u8(raw, h, M, P, K, True)
    else:
        x = oracle.synth_iq(SEED, 0, sum(lens))
        d, want = gpu.from_numpy(x).cuda(), ref.spectrum(x, h, M, P, K, True)
    s = redio.Stream(plan, u8=u8)
    e = 2 if u8 else 1
    for attempt in range(2):  # reset() starts over: the second pass repeats the first
        pos, outs, made = 0, [], 0
        for n in lens:
            expect = ref.nrows(pos + n, M, P, K) - made
            assert s.nout(n) == expect * M
            outs.append(s(d[e * pos: e * (pos + n)]).clone())
            pos += n
            made += expect
            assert s.pending == pos - made * H
        assert np.array_equal(bits(gpu.cat(outs).cpu().numpy()), bits(want.reshape(-1))), attempt
        s.reset()
        assert s.pending == 0
