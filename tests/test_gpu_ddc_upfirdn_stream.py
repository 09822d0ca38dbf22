"""The tuned resampler as a stream (redio_ddc_upfirdn_stream_*): the resampler's whole periods with the tuner's carried phase -- any
segmentation of N samples gives the first U' * ((N - Wp) / D' + 1) outputs of one redio_ddc_upfirdn_enqueue on the whole stream with
first_index 0, bit for bit, from cf32 and from u8 bytes, on both routes; the index and the pending count hold after every piece."""
import ctypes as C

import numpy as np
import pytest

import ddc_upfirdn_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED17D2
FENCE = 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cuts(rng, n, Wp, Dp, style):
    out, left = [], n
    while left:
        if style == "tiny":     # pieces of 0 and 1 samples, pieces shorter than a period's new samples and shorter than the window
            k = int(rng.choice([0, 1, 1, 2, max(Dp - 1, 0), max(Wp - 1, 1), int(rng.integers(0, Wp + 2))]))
        elif style == "small":
            k = int(rng.integers(1, 900))
        else:                   # more than one tile among them
            k = int(rng.choice([0, 1, 7, Wp, Wp + 1, 1000, 4095, 4096, 4097, 20000]))
        k = min(left, k)
        out.append(k); left -= k
    return out


@pytest.fixture(scope="module")
def streams(oracle):
    """per (U, D, K, L, u8, length): the taps, the table, the input and the one-call outputs of both folds, computed once"""
    made = {}

    def get(U, D, K, L, u8, n):
        key = (U, D, K, L, u8, n)
        if key not in made:
            taps, w = oracle.synth_f32(5, K, K), oracle.synth_iq(7, L, L)
            raw = np.random.default_rng(SEED + K).integers(0, 256, 2 * n, dtype=np.uint8)
            xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, K, n)
            want = {f: ref.ddc_upfirdn(xh, w, taps, U, D, f, 0) for f in (False, True)}
            for a in want.values():
                a.setflags(write=False)
            made[key] = (taps, w, raw if u8 else xh, want)
        return made[key]
    return get


@pytest.mark.parametrize("style", ["tiny", "small", "mixed"])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("U,D,K,L,fused", [(2, 1, 63, 24, True), (3, 2, 64, 4099, False), (4, 5, 100, 3, True),      # route 1
                                           (2, 7, 9, 24, True), (160, 147, 481, 65536, False)])                      # route 2
def test_any_segmentation_is_the_prefix_of_the_one_call_result(gpu, redio, streams, U, D, K, L, fused, u8, style):
    rng = np.random.default_rng(K * 131 + D + U)
    Up, Dp = ref.periods(U, D)
    Wp = ref.window(K, U, D)
    n = max(1500, Wp + 1500) if style == "tiny" else 30000
    E = 2 if u8 else 1
    taps, w, xh, want = streams(U, D, K, L, u8, n)
    total = Up * ((n - Wp) // Dp + 1)
    assert total <= len(want[fused])
    want = want[fused][:total]
    x = gpu.from_numpy(xh).cuda()
    plan = redio.DdcUpfirdn(w, taps, U, D, fused=fused)
    assert plan.route == ref.route(K, U, D)
    st = redio.Stream(plan, u8=u8)
    # the outputs land in one buffer, a fence of NaN behind every call's share: an extra output would overwrite it
    out = gpu.full((total + FENCE,), float("nan"), dtype=gpu.complex64, device="cuda")
    pos = done = 0
    assert st.index == 0 and st.pending == 0
    for k in cuts(rng, n, Wp, Dp, style):
        expect = st.nout(k)
        assert expect % Up == 0
        y = st(x[E * pos: E * (pos + k)], out=out[done:])
        assert y.numel() == expect
        pos += k; done += expect
        assert st.index == pos
        assert st.pending == pos - (done // Up) * Dp if Wp > Dp else st.pending < Wp
    got = out.cpu().numpy()
    assert done == total and np.isnan(got[total:]).all()  # nothing behind the last period (a complex fence is nan + 0j)
    assert np.array_equal(bits(got[:total]), bits(want)), (U, D, K, style)
    one = (plan.from_bytes if u8 else plan)(x, first=0).cpu().numpy()
    assert len(one) >= total and np.array_equal(bits(one[:total]), bits(want))
    # reset forgets the history and the phase
    st.reset()
    assert st.pending == 0 and st.index == 0
    half = n // 2 + 1
    again = gpu.cat([st(x[: E * half]).clone(), st(x[E * half:]).clone()]).cpu().numpy()
    assert np.array_equal(bits(again), bits(want)) and st.index == n


@pytest.mark.parametrize("u8", [False, True])
def test_a_failed_call_keeps_the_state(gpu, redio, oracle, u8):
    L = redio.lib()
    U, D, K, E = 3, 2, 64, 2 if u8 else 1
    taps, w = oracle.synth_f32(5, K, K), oracle.synth_iq(7, 24, 24)
    xh = np.random.default_rng(SEED).integers(0, 256, 12000, dtype=np.uint8) if u8 else oracle.synth_iq(SEED, 2, 6000)
    plan = redio.DdcUpfirdn(w, taps, U, D)
    st = redio.Stream(plan, u8=u8)
    x = gpu.from_numpy(xh).cuda()
    stream = redio.current_stream()
    a = st(x[: E * 1000]).clone()
    pending, index = st.pending, st.index
    assert index == 1000
    got = C.c_size_t(7)
    # outputs are due and there is no output buffer: refused, nothing moves
    assert st.nout(100) > 0
    assert L.redio_ddc_upfirdn_stream_enqueue(st._h, C.c_void_p(x.data_ptr()), 100, None, C.byref(got), stream) == -1 and got.value == 0
    assert (st.pending, st.index) == (pending, index)
    assert L.redio_ddc_upfirdn_stream_enqueue(st._h, None, 100, C.c_void_p(a.data_ptr()), C.byref(got), stream) == -1
    assert (st.pending, st.index) == (pending, index)
    b = st(x[E * 1000:]).clone()
    want = (plan.from_bytes if u8 else plan)(x)
    both = gpu.cat([a, b])
    assert np.array_equal(bits(both.cpu().numpy()), bits(want[: both.numel()].cpu().numpy()))
    assert both.numel() == 3 * ((6000 - ref.window(K, U, D)) // 2 + 1) and st.index == 6000
