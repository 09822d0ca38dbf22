"""The rational resampler (redio_upfirdn_*: up, FIR, down as a polyphase FIR over the original samples) on the device, bit for bit against
the per-phase reference built from the oracle's FIR (tests/upfirdn_ref.py) and against the route it replaces on the device itself
(redio_fir on a zero-stuffed tensor)."""
import numpy as np
import pytest

import upfirdn_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EEDF1D1
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.5, 2.0 ** -126, -(2.0 ** -126), 2.0 ** 127], np.float32)  # the ladder of test_gpu_ddc.py

# (U, D, K)
ROUTE1 = [(2, 1, 63), (3, 2, 64), (2, 3, 31), (4, 5, 100), (5, 4, 127), (16, 1, 255), (3, 8, 17), (7, 10, 40),
          (6, 4, 50),    # gcd 2
          (5, 1, 3),     # K < U: phases without taps
          (1, 5, 127)]   # U' = 1: redio_fir itself
ROUTE2 = [(160, 147, 481), (3, 16, 33), (17, 1, 40), (2, 7, 9)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_special(got, want):
    """bit for bit, NaNs by position (as test_gpu_ddc.py)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


def synth(oracle, cplx, first, n):
    return oracle.synth_iq(SEED, first, n) if cplx else oracle.synth_f32(SEED, first, n)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("U,D,K,route", [s + (1,) for s in ROUTE1] + [s + (2,) for s in ROUTE2])
def test_one_shot_against_the_reference(gpu, redio, oracle, U, D, K, route, cplx, fused):
    """Output counts around the tile: for each target in 0, 1, T - 1, T, T + 1, 2T + 1 (T one workgroup's outputs) the shortest input
    that yields at least that many -- with U > D a call cannot yield every count, it then yields fewer than U / D more -- and every
    output the call has is compared.  Then input and output at aligned addresses and one sample off."""
    T = ref.tile_out(K, U, D)
    assert 256 <= T <= 256 * 4 * 16  # at most 4 periods per lane of at most 16 outputs
    taps = oracle.synth_f32(3, K, K)
    plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)
    Up, Dp = ref.periods(U, D)
    assert plan.route == route == ref.route(K, U, D)
    assert (plan.period_out, plan.period_in, plan.window) == (Up, Dp, ref.window(K, U, D))
    targets = [0, 1, T - 1, T, T + 1, 2 * T + 1]
    nmax = ref.n_for(targets[-1], K, U, D)
    xh = synth(oracle, cplx, K + D, nmax)
    want = ref.upfirdn(xh, taps, U, D, fused)
    dt = gpu.complex64 if cplx else gpu.float32
    buf = gpu.zeros(nmax + 4, dtype=dt, device="cuda")
    views = {}
    for off in (0, 1):
        b = buf.clone()
        b[off: off + nmax] = gpu.from_numpy(xh).cuda()
        views[off] = b[off: off + nmax]
    for target in targets:
        n = (K - 1) // U if target == 0 else ref.n_for(target, K, U, D)
        n_out = ref.nout(n, K, U, D)
        assert plan.nout(n) == n_out and target <= n_out < target + -(-U // D) and (target or n_out == 0)
        got = plan(views[0][:n])
        assert got.numel() == n_out
        assert np.array_equal(bits(got.cpu().numpy()), bits(want[:n_out])), target
    obuf = gpu.empty(len(want) + 2, dtype=dt, device="cuda")
    for off, ooff in [(0, 1), (1, 0), (1, 1)]:
        got = plan(views[off], out=obuf[ooff:])
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (off, ooff)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
def test_no_interpolation_is_the_fir_itself(gpu, redio, oracle, cplx, fused):
    U, D, K = 1, 5, 127
    n = ref.n_for(3 * ref.tile_out(K, U, D) + 7, K, U, D)
    taps, xh = oracle.synth_f32(3, K, K), synth(oracle, cplx, 5, n)
    x = gpu.from_numpy(xh).cuda()
    want = redio.Fir(taps, D, complex_input=cplx, fused=fused)(x)
    got = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)(x)
    assert got.numel() == want.numel() == (n - K) // D + 1
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("U,D,K", [(3, 2, 64), (2, 3, 31), (17, 1, 40)])
def test_equals_the_route_before_this_plan_on_the_device(gpu, redio, oracle, U, D, K, fused):
    """Upfirdn(x) against redio_fir(taps, D) on a zero-stuffed tensor, three tiles: both computed by the library.  Equal on these inputs
    (no product underflows and nothing is infinite), which is where the two definitions may part."""
    n = ref.n_for(3 * ref.tile_out(K, U, D) + 7, K, U, D)
    taps, xh = oracle.synth_f32(3, K, K), oracle.synth_iq(SEED, 5, n)
    x = gpu.from_numpy(xh).cuda()
    z = gpu.zeros(n * U, dtype=gpu.complex64, device="cuda")
    z[::U] = x
    want = redio.Fir(taps, D, complex_input=True, fused=fused)(z)
    got = redio.Upfirdn(taps, U, D, complex_input=True, fused=fused)(x)
    assert got.numel() == want.numel() == ref.nout(n, K, U, D)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


def special_inputs(oracle, U, D, K, cplx):
    """three tiles of samples with every value of the ladder in them (each at several random places), and taps with a few random
    ladder values: a NaN or infinite tap poisons only the phases it belongs to"""
    rng = np.random.default_rng(SEED + K)
    n = ref.n_for(3 * ref.tile_out(K, U, D), K, U, D)
    xh, taps = synth(oracle, cplx, 9, n).copy(), oracle.synth_f32(3, K, K).copy()
    f = xh.view(np.float32).reshape(-1)
    k = max(3 * len(SPECIALS), int(0.002 * len(f)))
    f[rng.choice(len(f), k, replace=False)] = SPECIALS[np.arange(k) % len(SPECIALS)]
    k = max(1, int(0.03 * K))
    taps[rng.integers(0, K, k)] = SPECIALS[rng.integers(0, len(SPECIALS), k)]
    return xh, taps


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("U,D,K", [(2, 1, 63), (4, 5, 100), (5, 1, 3), (160, 147, 481)])
def test_special_values_through_the_fold(gpu, redio, oracle, U, D, K, cplx, fused):
    xh, taps = special_inputs(oracle, U, D, K, cplx)
    want = ref.upfirdn(xh, taps, U, D, fused)
    got = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)(gpu.from_numpy(xh).cuda()).cpu().numpy()
    assert np.isnan(want.view(np.float32)).any() and np.isfinite(want.view(np.float32)).any()
    assert same_special(got, want)


def test_forty_random_cases(gpu, redio, oracle):
    rng = np.random.default_rng(SEED)
    routes = set()
    for case in range(40):
        U, D, K = int(rng.integers(1, 25)), int(rng.integers(1, 25)), int(rng.integers(1, 401))
        n = int(rng.integers(0, 2 ** 16 + 1))
        cplx, fused = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        taps, xh = oracle.synth_f32(case, 0, K), synth(oracle, cplx, case, n)
        plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)
        assert plan.route == ref.route(K, U, D)
        routes.add(plan.route)
        want = ref.upfirdn(xh, taps, U, D, fused)
        got = plan(gpu.from_numpy(xh).cuda())
        assert got.numel() == len(want) == plan.nout(n), (case, U, D, K, n)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (case, U, D, K, n, cplx, fused)
    assert routes == {1, 2}
