"""The tuner (redio_ddc_*: oscillator mix fused into the FIR tile load) on the device, bit for bit against the oracle's mul_vecs + fir
(tests/ddc_ref.py) and against the route it replaces on the device itself (redio_mul_c32 on a materialised oscillator, then redio_fir)."""
import numpy as np
import pytest

import ddc_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EEDDDC1
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.5, 2.0 ** -126, -(2.0 ** -126), 2.0 ** 127], np.float32)  # the ladder of test_gpu_special_values.py


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_special(got, want):
    """bit for bit, NaNs by position (as test_gpu_special_values.py)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


def table(oracle, L):
    return ref.osc_table_ref(-5, 24) if L == 24 else oracle.synth_iq(7, L, L)


SPECIALISED = [(127, 5), (63, 5), (63, 1), (127, 1)]
CHUNKED = [(31, 2), (17, 3), (100, 4), (255, 10), (64, 8), (1, 1)]
DIRECT = [(5, 9), (33, 7)]
PERIODS = [1, 2, 3, 4, 24, 1000, 4099, 65536]


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("K,D,route", [(k, d, 1) for k, d in SPECIALISED] + [(k, d, 2) for k, d in CHUNKED] + [(k, d, 3) for k, d in DIRECT])
def test_one_shot_against_the_oracle(gpu, redio, oracle, K, D, route, fused, u8):
    rng = np.random.default_rng(SEED + 977 * K + 31 * D + 2 * fused + u8)
    TO = ref.tile_out(K, D)
    assert 256 <= TO <= 2048
    nouts = [0, 1, TO - 1, TO, TO + 1, 2 * TO + 1]
    nmax = (nouts[-1] - 1) * D + K
    taps = oracle.synth_f32(3, K, K)
    raw = rng.integers(0, 256, 2 * nmax, dtype=np.uint8)
    xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, K + D, nmax)
    src = raw if u8 else xh
    E = 2 if u8 else 1
    # the samples once, at an aligned address and behind an offset of one sample (cf32: 8 bytes, u8: two bytes) and, for u8, of one byte
    buf = gpu.zeros(len(src) + 4 * E, dtype=gpu.uint8 if u8 else gpu.complex64, device="cuda")
    views = {}
    for off in ([0, 2, 1] if u8 else [0, 1]):
        b = buf.clone()
        b[off: off + len(src)] = gpu.from_numpy(src).cuda()
        views[off] = b[off: off + len(src)]
    obuf = gpu.empty(nouts[-1] + 2, dtype=gpu.complex64, device="cuda")
    for L in PERIODS:
        w = table(oracle, L)
        plan = redio.Ddc(w, taps, D, fused=fused)
        assert plan.route == route == ref.route(K, D) and plan.period == L
        for first in [0, 1, L - 1, 2 ** 32 + 5]:
            want = ref.ddc(xh, w, taps, D, fused, first)
            assert len(want) == nouts[-1]
            for n_out in nouts:
                n = K - 1 if n_out == 0 else (n_out - 1) * D + K
                assert plan.nout(n) == n_out
                x = views[0][: E * n]
                got = (plan.from_bytes if u8 else plan)(x, first=first)
                assert got.numel() == n_out
                assert np.array_equal(bits(got.cpu().numpy()), bits(want[:n_out])), (L, first, n_out)
        # unaligned pointers, in and out: the slower paths, the same bits
        for off, ooff in [(o, oo) for o in views for oo in (0, 1)]:
            n = (nouts[-1] - 1) * D + K
            got = (plan.from_bytes if u8 else plan)(views[off][: E * n], first=first, out=obuf[ooff:])
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (L, off, ooff)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("K,D", [(127, 5), (31, 2)])
def test_equals_the_route_before_this_plan_on_the_device(gpu, redio, oracle, K, D, fused):
    """Ddc(x) against redio_fir on redio_mul_c32(x, the table tiled from first): both computed by the library"""
    TO = ref.tile_out(K, D)
    n_out, first, L = 3 * TO + 7, 12345, 4099
    n = (n_out - 1) * D + K
    taps, w = oracle.synth_f32(3, K, K), table(oracle, L)
    x = gpu.from_numpy(oracle.synth_iq(SEED, 5, n)).cuda()
    osc = gpu.from_numpy(ref.tiled(w, first, n)).cuda()
    m = gpu.empty_like(x)
    from libredio_amd.plans import _dev_ptr, current_stream
    redio.check(redio.lib().redio_mul_c32(_dev_ptr(x), _dev_ptr(osc), _dev_ptr(m), n, current_stream()), "mul_c32")
    want = redio.Fir(taps, D, complex_input=True, fused=fused)(m)
    got = redio.Ddc(w, taps, D, fused=fused)(x, first=first)
    assert got.numel() == want.numel() == n_out
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("K,D", [(127, 5), (63, 1), (100, 4), (33, 7)])
def test_special_values_through_the_mix_and_the_fold(gpu, redio, oracle, K, D, fused):
    rng = np.random.default_rng(SEED + K)
    n, L, first = 3 * ref.tile_out(K, D) * D + K, 1000, 77
    xh, w, taps = oracle.synth_iq(SEED, 9, n), table(oracle, L).copy(), oracle.synth_f32(3, K, K).copy()
    for a, density in ((xh, 0.002), (w, 0.01), (taps, 0.03)):
        f = a.view(np.float32).reshape(-1)
        k = max(1, int(density * len(f)))
        f[rng.integers(0, len(f), k)] = SPECIALS[rng.integers(0, len(SPECIALS), k)]
    want = ref.ddc(xh, w, taps, D, fused, first)
    got = redio.Ddc(w, taps, D, fused=fused)(gpu.from_numpy(xh).cuda(), first=first).cpu().numpy()
    assert np.isnan(want.view(np.float32)).any() and np.isfinite(want.view(np.float32)).any()
    assert same_special(got, want)


@pytest.mark.parametrize("num", [1, -1])
@pytest.mark.parametrize("K,D", [(127, 5), (31, 2), (5, 9)])
def test_quarter_rate_shift_is_exact(gpu, redio, oracle, K, D, num):
    """the fs/4 table holds 1, i, -1, -i exactly: the mix only permutes and negates components, so the outputs are a FIR over samples
    rearranged on the host -- no rounding in the mix"""
    w = redio.dsputils.osc_table(num, 4)
    assert np.array_equal(w, np.array([1, 1j, -1, -1j] if num == 1 else [1, -1j, -1, 1j], np.complex64))
    n, first = 2 * ref.tile_out(K, D) * D + K + 3, 6
    xh = oracle.synth_iq(SEED, 11, n)
    assert (xh.real != 0).all() and (xh.imag != 0).all()
    q = ((first + np.arange(n)) * (1 if num == 1 else 3)) % 4  # the quarter turns applied to sample n
    re = np.choose(q, [xh.real, -xh.imag, -xh.real, xh.imag])
    im = np.choose(q, [xh.imag, xh.real, -xh.imag, -xh.real])
    m = (re + 1j * im).astype(np.complex64)
    taps = oracle.synth_f32(3, K, K)
    want = oracle.fir(m, taps, D, True)
    got = redio.Ddc(w, taps, D, fused=True)(gpu.from_numpy(xh).cuda(), first=first).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))


def test_forty_random_cases(gpu, redio, oracle):
    rng = np.random.default_rng(SEED)
    for case in range(40):
        K, D, L = int(rng.integers(1, 301)), int(rng.integers(1, 13)), int(rng.integers(1, 65537))
        first, n = int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 16 + 1))
        u8, fused = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
        taps, w = oracle.synth_f32(case, 0, K), oracle.synth_iq(case, 1, L)
        plan = redio.Ddc(w, taps, D, fused=fused)
        assert plan.route == ref.route(K, D)
        if u8:
            raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
            want = ref.ddc_u8(raw, w, taps, D, fused, first)
            got = plan.from_bytes(gpu.from_numpy(raw).cuda(), first=first)
        else:
            xh = oracle.synth_iq(SEED, case, n)
            want = ref.ddc(xh, w, taps, D, fused, first)
            got = plan(gpu.from_numpy(xh).cuda(), first=first)
        assert got.numel() == len(want) == plan.nout(n), (case, K, D, L, n)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (case, K, D, L, first, n, u8, fused)
