"""The tuned resampler (redio_ddc_upfirdn_*: the tuner's oscillator mix fused into the rational resampler's tile load) on the device, bit
for bit against the reference built from the oracle's own blocks (tests/ddc_upfirdn_ref.py), against the route it replaces on the device
itself (redio_mul_c32 on a materialised oscillator, then redio_upfirdn) and, without interpolation, against the tuner."""
import numpy as np
import pytest

import ddc_ref
import ddc_upfirdn_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED17D1
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.5, 2.0 ** -126, -(2.0 ** -126), 2.0 ** 127], np.float32)  # the ladder of test_gpu_upfirdn.py

# (U, D, K)
ROUTE1 = [(2, 1, 63), (3, 2, 64), (2, 3, 31), (4, 5, 100), (3, 8, 17), (7, 10, 40),
          (6, 4, 50),    # gcd 2
          (5, 1, 3),     # K < U: phases without taps
          (1, 5, 127)]   # U' = 1: the tuner itself
ROUTE2 = [(160, 147, 481), (3, 16, 33), (2, 7, 9)]
PERIODS = (1, 3, 24, 65536)
RANDOM_SEED = 0x5EED17D5  # chosen on the CPU with upfirdn_ref.route: its forty cases take route 1 and route 2 (test_forty_random_cases)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_special(got, want):
    """bit for bit, NaNs by position (as test_gpu_upfirdn.py)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


def table(oracle, L):
    return oracle.synth_iq(7, L, L)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("U,D,K,route", [s + (1,) for s in ROUTE1] + [s + (2,) for s in ROUTE2])
def test_one_shot_against_the_reference(gpu, redio, oracle, U, D, K, route, u8, fused):
    """Output counts around the tile: for each target in 0, 1, T - 1, T, T + 1, 2T + 1 (T one workgroup's outputs) the shortest input that
    yields at least that many, every output compared (an output depends on the samples in front of its window's end only, so the
    reference of the longest input serves them all); oscillator periods 1, 3, 24, 65536 times first in {0, L - 1, 2^40 + 3}.  Then input
    and output at aligned addresses and one sample off, bytes at offsets 0 to 3."""
    T = ref.tile_out(K, U, D)
    assert 256 <= T <= 16384
    taps = oracle.synth_f32(3, K, K)
    Up, Dp = ref.periods(U, D)
    targets = [0, 1, T - 1, T, T + 1, 2 * T + 1]
    nmax = ref.n_for(targets[-1], K, U, D)
    E = 2 if u8 else 1
    raw = np.random.default_rng(SEED + K).integers(0, 256, 2 * nmax, dtype=np.uint8)
    xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, K + D, nmax)
    src = gpu.from_numpy(raw if u8 else xh).cuda()
    views = {}
    for off in range(4 if u8 else 2):   # bytes: every byte offset; cf32: on a 16-byte boundary and one sample off
        b = gpu.zeros(E * nmax + 4, dtype=src.dtype, device="cuda")
        b[off: off + E * nmax] = src
        views[off] = b[off: off + E * nmax]
    obuf = gpu.empty(ref.nout(nmax, K, U, D) + 2, dtype=gpu.complex64, device="cuda")
    for L in PERIODS:
        w = table(oracle, L)
        plan = redio.DdcUpfirdn(w, taps, U, D, fused=fused)
        run = plan.from_bytes if u8 else plan
        assert plan.route == route == ref.route(K, U, D) and plan.period == L
        assert (plan.period_out, plan.period_in, plan.window) == (Up, Dp, ref.window(K, U, D))
        for first in (0, L - 1, 2 ** 40 + 3):
            want = ref.ddc_upfirdn(xh, w, taps, U, D, fused, first)
            for target in targets:
                n = (K - 1) // U if target == 0 else ref.n_for(target, K, U, D)
                n_out = ref.nout(n, K, U, D)
                assert plan.nout(n) == n_out and target <= n_out < target + -(-U // D) and (target or n_out == 0)
                got = run(views[0][: E * n], first=first)
                assert got.numel() == n_out
                assert np.array_equal(bits(got.cpu().numpy()), bits(want[:n_out])), (L, first, target)
        # first = 2^40 + 3: every input offset against both output offsets in turn
        # first = 2^40 + 3: the other input offsets, and the output one sample off a 16-byte boundary
        for off, ooff in ([(0, 1), (1, 0), (2, 1), (3, 0), (1, 1)] if u8 else [(0, 1), (1, 0), (1, 1)]):
            got = run(views[off], first=first, out=obuf[ooff:])
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (L, off, ooff)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("U,D,K", [(3, 2, 64), (2, 3, 31), (160, 147, 481)])
def test_equals_the_route_before_this_plan_on_the_device(gpu, redio, oracle, U, D, K, u8, fused):
    """DdcUpfirdn(x) against redio_upfirdn on redio_mul_c32(x, the table tiled from first) -- from bytes behind redio_data_to_samples --
    three tiles, all computed by the library"""
    from libredio_amd.plans import _dev_ptr, current_stream
    first, L = 12345, 4099
    n = ref.n_for(3 * ref.tile_out(K, U, D) + 7, K, U, D)
    taps, w = oracle.synth_f32(3, K, K), table(oracle, L)
    if u8:
        raw = gpu.from_numpy(np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8)).cuda()
        x = redio.bitfount.data_to_samples(raw)
    else:
        x = gpu.from_numpy(oracle.synth_iq(SEED, 5, n)).cuda()
    osc = gpu.from_numpy(ddc_ref.tiled(w, first, n)).cuda()
    m = gpu.empty_like(x)
    redio.check(redio.lib().redio_mul_c32(_dev_ptr(x), _dev_ptr(osc), _dev_ptr(m), n, current_stream()), "mul_c32")
    want = redio.Upfirdn(taps, U, D, complex_input=True, fused=fused)(m)
    plan = redio.DdcUpfirdn(w, taps, U, D, fused=fused)
    got = plan.from_bytes(raw, first=first) if u8 else plan(x, first=first)
    assert got.numel() == want.numel() == ref.nout(n, K, U, D)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("D,K", [(5, 127), (2, 31)])
def test_no_interpolation_is_the_tuner_itself(gpu, redio, oracle, D, K, u8, fused):
    first, L = 2 ** 33 + 1, 1000
    n = ref.n_for(3 * ref.tile_out(K, 1, D) + 7, K, 1, D)
    taps, w = oracle.synth_f32(3, K, K), table(oracle, L)
    xh = np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8) if u8 else oracle.synth_iq(SEED, 5, n)
    x = gpu.from_numpy(xh).cuda()
    tuner, plan = redio.Ddc(w, taps, D, fused=fused), redio.DdcUpfirdn(w, taps, 1, D, fused=fused)
    want = (tuner.from_bytes if u8 else tuner)(x, first=first)
    got = (plan.from_bytes if u8 else plan)(x, first=first)
    assert got.numel() == want.numel() == (n - K) // D + 1
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("U,D,K", [(2, 1, 63), (4, 5, 100), (5, 1, 3), (160, 147, 481)])
def test_special_values_through_the_mix_and_the_fold(gpu, redio, oracle, U, D, K, fused):
    """three tiles of samples with every value of the ladder in them, and a few ladder values in the taps and in the table"""
    rng = np.random.default_rng(SEED + K)
    n, L, first = ref.n_for(3 * ref.tile_out(K, U, D), K, U, D), 1000, 77
    xh, w, taps = oracle.synth_iq(SEED, 9, n).copy(), table(oracle, L).copy(), oracle.synth_f32(3, K, K).copy()
    f = xh.view(np.float32).reshape(-1)
    k = max(3 * len(SPECIALS), int(0.002 * len(f)))
    f[rng.choice(len(f), k, replace=False)] = SPECIALS[np.arange(k) % len(SPECIALS)]
    for a, density in ((w, 0.01), (taps, 0.03)):
        f = a.view(np.float32).reshape(-1)
        k = max(1, int(density * len(f)))
        f[rng.integers(0, len(f), k)] = SPECIALS[rng.integers(0, len(SPECIALS), k)]
    want = ref.ddc_upfirdn(xh, w, taps, U, D, fused, first)
    got = redio.DdcUpfirdn(w, taps, U, D, fused=fused)(gpu.from_numpy(xh).cuda(), first=first).cpu().numpy()
    assert np.isnan(want.view(np.float32)).any() and np.isfinite(want.view(np.float32)).any()
    assert same_special(got, want)


def random_cases():
    rng = np.random.default_rng(RANDOM_SEED)
    for case in range(40):
        U, D, K = int(rng.integers(1, 25)), int(rng.integers(1, 25)), int(rng.integers(1, 401))
        n, L = int(rng.integers(0, 2 ** 16 + 1)), int(rng.integers(1, 1001))
        first = int(rng.integers(0, 2 ** 63))
        u8, fused = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        yield case, U, D, K, n, L, first, u8, fused


def test_forty_random_cases(gpu, redio, oracle):
    routes = set()
    for case, U, D, K, n, L, first, u8, fused in random_cases():
        taps, w = oracle.synth_f32(case, 0, K), table(oracle, L)
        raw = np.random.default_rng(case).integers(0, 256, 2 * n, dtype=np.uint8)
        xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, case, n)
        plan = redio.DdcUpfirdn(w, taps, U, D, fused=fused)
        assert plan.route == ref.route(K, U, D)
        routes.add(plan.route)
        want = ref.ddc_upfirdn(xh, w, taps, U, D, fused, first)
        got = plan.from_bytes(gpu.from_numpy(raw).cuda(), first=first) if u8 else plan(gpu.from_numpy(xh).cuda(), first=first)
        assert got.numel() == len(want) == plan.nout(n), (case, U, D, K, n)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (case, U, D, K, n, L, first, u8, fused)
    assert routes == {1, 2}
