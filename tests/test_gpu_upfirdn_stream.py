"""The rational resampler as a stream (redio_upfirdn_stream_*): whole periods -- any segmentation of N samples gives the first
U' * ((N - Wp) / D' + 1) outputs of one redio_upfirdn_enqueue on the whole stream, bit for bit, and not one output more (with U > D a
stateless call on the same samples would write a few)."""
import ctypes as C

import numpy as np
import pytest

import upfirdn_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EEDF1D2
FENCE = 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cuts(rng, n, Wp, style):
    if style == "one":
        return [n]
    out, left = [], n
    while left:
        if style == "tiny":     # pieces of 0 and 1 samples and pieces shorter than the window
            k = int(rng.choice([0, 1, 1, 2, max(Wp - 1, 1), int(rng.integers(0, Wp + 2))]))
        elif style == "small":
            k = int(rng.integers(1, 900))
        else:
            k = int(rng.choice([1, 7, Wp, Wp + 1, 1000, 4095, 4096, 4097, 20000]))
        k = min(left, k)
        out.append(k); left -= k
    return out


@pytest.fixture(scope="module")
def streams(oracle):
    """per (U, D, K, complex, length): the taps, the input and the one-call outputs of both folds, computed once"""
    made = {}

    def get(U, D, K, cplx, n):
        key = (U, D, K, cplx, n)
        if key not in made:
            taps = oracle.synth_f32(5, K, K)
            xh = oracle.synth_iq(SEED, K, n) if cplx else oracle.synth_f32(SEED, K, n)
            want = {f: ref.upfirdn(xh, taps, U, D, f) for f in (False, True)}
            for a in want.values():
                a.setflags(write=False)
            made[key] = (taps, xh, want)
        return made[key]
    return get


@pytest.mark.parametrize("style", ["one", "tiny", "small", "mixed"])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("U,D,K,fused", [(2, 1, 63, True), (3, 2, 64, False), (16, 1, 255, True), (17, 1, 40, False), (2, 7, 9, True),
                                         (2, 1, 11776, False)])  # a window of 5889 samples in a tile of 85536 bytes
def test_any_segmentation_is_the_prefix_of_the_one_call_result(gpu, redio, streams, U, D, K, fused, cplx, style):
    rng = np.random.default_rng(K * 131 + D + U)
    Up, Dp = ref.periods(U, D)
    Wp = ref.window(K, U, D)
    n = max(1500, Wp + 1500) if style == "tiny" else 30000  # the long window: 1500 samples behind it
    taps, xh, want = streams(U, D, K, cplx, n)
    total = Up * ((n - Wp) // Dp + 1)
    assert total <= len(want[fused])
    want = want[fused][:total]
    x = gpu.from_numpy(xh).cuda()
    plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)
    st = redio.Stream(plan)
    # the outputs land in one buffer, a fence of NaN behind every call's share: an extra output would overwrite it
    dt = gpu.complex64 if cplx else gpu.float32
    out = gpu.full((total + FENCE,), float("nan"), dtype=dt, device="cuda")
    pos = done = 0
    for k in cuts(rng, n, Wp, style):
        expect = st.nout(k)
        assert expect % Up == 0
        y = st(x[pos: pos + k], out=out[done:])
        assert y.numel() == expect
        pos += k; done += expect
    got = out.cpu().numpy()
    assert done == total and np.isnan(got[total:]).all()  # nothing behind the last period (a complex fence is nan + 0j)
    assert np.array_equal(bits(got[:total]), bits(want)), (U, D, K, style)
    assert st.pending == n - (total // Up) * Dp if Wp > Dp else st.pending < Wp
    one = plan(x).cpu().numpy()
    assert len(one) >= total and np.array_equal(bits(one[:total]), bits(want))
    # reset forgets the history
    st.reset()
    assert st.pending == 0
    half = n // 2 + 1
    again = gpu.cat([st(x[:half]).clone(), st(x[half:]).clone()]).cpu().numpy()
    assert np.array_equal(bits(again), bits(want))


@pytest.mark.parametrize("U,D,K", [(16, 1, 255), (5, 1, 3), (17, 1, 40)])
def test_a_body_call_writes_whole_periods_only(gpu, redio, oracle, U, D, K):
    """one piece on a fresh stream is one body run; the stateless call on it has 2, 3 and 12 outputs more, which must not be written"""
    n = 5000
    taps, xh = oracle.synth_f32(5, K, K), oracle.synth_f32(SEED, 1, n)
    plan = redio.Upfirdn(taps, U, D)
    st = redio.Stream(plan)
    total = st.nout(n)
    Wp = ref.window(K, U, D)
    assert total == U * (n - Wp + 1) and plan.nout(n) - total == {255: 2, 3: 3, 40: 12}[K]
    out = gpu.full((total + FENCE,), float("nan"), dtype=gpu.float32, device="cuda")
    y = st(gpu.from_numpy(xh).cuda(), out=out)
    assert y.numel() == total
    got = out.cpu().numpy()
    assert np.isnan(got[total:]).all()
    assert np.array_equal(bits(got[:total]), bits(ref.upfirdn(xh, taps, U, D)[:total]))


def test_a_failed_call_keeps_the_state(gpu, redio, oracle):
    L = redio.lib()
    U, D, K = 3, 2, 64
    taps, xh = oracle.synth_f32(5, K, K), oracle.synth_iq(SEED, 2, 6000)
    plan = redio.Upfirdn(taps, U, D, complex_input=True)
    st = redio.Stream(plan)
    x = gpu.from_numpy(xh).cuda()
    stream = redio.current_stream()
    a = st(x[:1000]).clone()
    pending = st.pending
    got = C.c_size_t(7)
    # outputs are due and there is no output buffer: refused, nothing moves
    assert st.nout(100) > 0
    assert L.redio_upfirdn_stream_enqueue(st._h, C.c_void_p(x.data_ptr()), 100, None, C.byref(got), stream) == -1 and got.value == 0
    assert st.pending == pending
    assert L.redio_upfirdn_stream_enqueue(st._h, None, 100, C.c_void_p(a.data_ptr()), C.byref(got), stream) == -1
    assert st.pending == pending
    b = st(x[1000:]).clone()
    want = plan(x)
    both = gpu.cat([a, b])
    assert np.array_equal(bits(both.cpu().numpy()), bits(want[: both.numel()].cpu().numpy()))
    assert both.numel() == 3 * ((6000 - ref.window(K, U, D)) // 2 + 1)
