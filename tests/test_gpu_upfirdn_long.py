"""The rational resampler (redio_upfirdn_*) on the device at long filters and extreme ratios, bit for bit against the per-phase reference
(tests/upfirdn_ref.py): every kernel instantiation route 1 can launch, in both passes of upfirdn_r (tiles inside 52 KiB, and of 52 to
150 KiB through hipFuncSetAttribute), the hand-over to route 2 at the LDS limit, every chunk remainder, windows of thousands of
samples with infinities on either side of them, and route 2 at create's limits.  The oracle's cost is outputs x taps per phase, so
every case asks for one whole tile and a partial one and never shortens the filter."""
import math

import numpy as np
import pytest

import upfirdn_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EEDF1D4


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


def synth(oracle, cplx, first, n):
    return oracle.synth_iq(SEED, first, n) if cplx else oracle.synth_f32(SEED, first, n)


def both_alignments(gpu, plan, xh, want):
    """the call on xh at a 16-byte boundary into one, and one sample off it into a buffer one sample off"""
    n, dt = len(xh), gpu.complex64 if plan.complex_input else gpu.float32
    assert plan.nout(n) == len(want)
    buf = gpu.zeros(n + 4, dtype=dt, device="cuda")
    obuf = gpu.empty(len(want) + 4, dtype=dt, device="cuda")
    for off in (0, 1):
        buf[off: off + n] = gpu.from_numpy(xh).cuda()
        assert (buf[off:].data_ptr() % 16 == 0) == (off == 0) and (obuf[off:].data_ptr() % 16 == 0) == (off == 0)
        got = plan(buf[off: off + n], out=obuf[off:])
        assert got.numel() == len(want)
        assert same_special(got.cpu().numpy(), want), off


def instantiations():
    """{(D', R, pass): (U', K)} over D' of the tiled set and U' in 2..16 coprime to it (U' >= 2: the phases differ): per kernel
    instantiation and pass of upfirdn_r the smallest K that selects it, at the smallest U' that has that K.  In the first pass that K
    is 1, which would run no whole chunk and leave phases without taps: the K taken there is 21 U', 21 taps in every phase (a whole
    16-tap chunk and the remainder's digits 4 and 1), where the regime holds it -- it always does, the first regime of every ratio here
    ends above 2000 taps."""
    found = {}
    for Dp in ref.TILED_D:
        for Up in range(2, ref.TILED_MAX_PERIOD_OUT + 1):
            if math.gcd(Up, Dp) != 1:
                continue
            rows = ref.regimes(Up, Dp)
            for (K, R, pas, route), nxt in zip(rows, rows[1:] + [(2 ** 20 + 1,)]):
                if route != 1:
                    continue
                if pas == 1 and K < 21 * Up < nxt[0]:
                    K = 21 * Up
                if (Dp, R, pas) not in found or K < found[(Dp, R, pas)][1]:
                    found[(Dp, R, pas)] = (Up, K)
    return found


# D' of 4 and 5 at R = 4 and D' = 10 at R = 2 fit 52 KiB at no U' >= 2 (their output tile alone is 256 R U' elements): they run in the
# second pass only.  Everything else the dispatcher holds, D' in {1, 2, 3, 4, 5} x R in {4, 2, 1} and D' in {8, 10} x R in {2, 1}, in
# both passes
REACHABLE = ({(Dp, R, pas) for Dp in (1, 2, 3, 4, 5) for R in (4, 2, 1) for pas in (1, 2)} |
             {(Dp, R, pas) for Dp in (8, 10) for R in (2, 1) for pas in (1, 2)}) - {(4, 4, 1), (5, 4, 1), (10, 2, 1)}


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
def test_every_instantiation_of_route_1_runs(gpu, redio, oracle, cplx, fused):
    """one whole tile and a partial one per (D', R, pass), aligned and one sample off; the set that ran is the reachable set"""
    found = instantiations()
    ran = set()
    for (Dp, R, pas), (Up, K) in sorted(found.items()):
        U, D = Up, Dp
        taps = oracle.synth_f32(3, K, K)
        plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)
        T = 256 * R * Up
        assert plan.route == ref.route(K, U, D) == 1 and ref.tile_out(K, U, D) == T and ref.lane_pass(K, U, D) == (R, pas)
        assert (plan.period_out, plan.period_in, plan.window) == (Up, Dp, ref.window(K, U, D))
        nbytes = ref.lds_elems(R, K, U, D) * 8
        assert nbytes <= ref.LDS_WANT if pas == 1 else ref.LDS_WANT < nbytes <= ref.LDS_MAX
        xh = synth(oracle, cplx, K + D, ref.n_for(T + 1 + 4, K, U, D))
        want = ref.upfirdn(xh, taps, U, D, fused)
        assert T + 5 <= len(want) < 2 * T
        both_alignments(gpu, plan, xh, want)
        ran.add((plan.period_in, ref.tile_out(K, U, D) // (256 * plan.period_out), pas))
    assert ran == REACHABLE == set(found)


@pytest.mark.parametrize("cplx,fused", [(False, True), (True, False)])
@pytest.mark.parametrize("U,D,K", [(2, 1, 36863), (3, 2, 39323), (4, 5, 67585), (3, 8, 43013), (16, 1, 237553)])
def test_the_hand_over_to_route_2(gpu, redio, oracle, U, D, K, cplx, fused):
    """the last tap count whose tile fits 150 KiB runs route 1, the next one route 2: the same bits on either side"""
    for k, route in ((K, 1), (K + 1, 2)):
        taps = oracle.synth_f32(3, k, k)
        plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)
        assert plan.route == route == ref.route(k, U, D)
        T = ref.tile_out(k, U, D)
        R = ref.periods_per_lane(k, U, D)  # the largest that fits: 2 at 3/2, 1 at the other ratios here
        assert T == (256 * R * ref.periods(U, D)[0] if route == 1 else 256) and (R > 0) == (route == 1)
        if route == 1:
            assert ref.lane_pass(k, U, D)[1] == 2 and all(ref.lds_elems(r, k + 1, U, D) * 8 > ref.LDS_MAX for r in (4, 2, 1))
        xh = synth(oracle, cplx, k + D, ref.n_for(T + 1 + 4, k, U, D))
        both_alignments(gpu, plan, xh, ref.upfirdn(xh, taps, U, D, fused))


@pytest.mark.parametrize("cplx,fused", [(False, False), (True, True)])
def test_every_chunk_remainder(gpu, redio, oracle, cplx, fused):
    """2/1 and 3/2 at every K from 2 to 70: sub-filters of 1 to 35 taps -- every remainder 0..15 behind zero, one and two whole chunks"""
    seen = set()
    for U, D in [(2, 1), (3, 2)]:
        T = ref.tile_out(2, U, D)
        for K in range(2, 71):
            assert ref.tile_out(K, U, D) == T and ref.route(K, U, D) == 1
            seen |= {(k // 16, k % 16) for _, _, k in ref.phases(K, U, D)}
            taps = oracle.synth_f32(3, K, K)
            xh = synth(oracle, cplx, K + U, ref.n_for(T + 1 + 4, K, U, D))
            want = ref.upfirdn(xh, taps, U, D, fused)
            got = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)(gpu.from_numpy(xh).cuda())
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (U, D, K)
    assert {(c, r) for c in (0, 1) for r in range(16)} - {(0, 0)} <= seen and {(2, 0), (2, 1), (2, 2), (2, 3)} <= seen


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
def test_no_tap_beyond_the_filter_is_multiplied_at_length(gpu, redio, oracle, cplx, fused):
    """2/1 at 11777 taps (R = 4 in the second pass; sub-filters of 5889 and 5888 taps, the first no multiple of 16): an infinity in the
    sample just before the window of output i and one in the sample just behind it leave output i the finite value it has without
    them; a NaN in the last tap poisons the phase it belongs to, and only that one"""
    U, D, K = 2, 1, 11777
    T = ref.tile_out(K, U, D)
    assert T == 2048 and ref.lane_pass(K, U, D) == (4, 2)
    taps = oracle.synth_f32(3, K, K)
    n = ref.n_for(T + 1 + 4, K, U, D)
    clean = synth(oracle, cplx, 7, n)
    want_clean = ref.upfirdn(clean, taps, U, D, fused)
    assert np.isfinite(want_clean.view(np.float32)).all()
    plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=fused)
    for i in (2, 1001, T - 1, T + 2):  # both phases; first and last lanes of the whole tile, the partial tile
        lo, hi = -(-(i * D) // U), (i * D + K - 1) // U  # the window of output i: samples lo..hi
        assert 1 <= lo and hi + 1 < n and hi - lo + 1 == ref.phases(K, U, D)[i % U][2]
        xh = clean.copy()
        xh[lo - 1] = xh[hi + 1] = np.inf
        want = ref.upfirdn(xh, taps, U, D, fused)
        got = plan(gpu.from_numpy(xh).cuda()).cpu().numpy()
        assert same_special(got, want)
        assert bits(got[i: i + 1]).tolist() == bits(want_clean[i: i + 1]).tolist() and not np.isfinite(want.view(np.float32)).all()
    bad = taps.copy()
    bad[K - 1] = np.nan  # tap 11776 = 0 + 2 * 5888: phase 0, the even outputs
    got = redio.Upfirdn(bad, U, D, complex_input=cplx, fused=fused)(gpu.from_numpy(clean).cuda()).cpu().numpy()
    assert same_special(got, ref.upfirdn(clean, bad, U, D, fused))
    assert np.isnan(np.ascontiguousarray(got[0::2]).view(np.float32)).all() and np.array_equal(bits(got[1::2]), bits(want_clean[1::2]))


def test_route_2_every_phase_of_the_largest_table(gpu, redio, oracle):
    """U = 65536 against D = 65535: U' = 65536 phases with sub-filters of 3 and 4 taps, every one of them used by 70000 samples"""
    U, D, K, n = 65536, 65535, 200000, 70000
    taps, xh = oracle.synth_f32(3, K, K), oracle.synth_iq(SEED, 1, n)
    plan = redio.Upfirdn(taps, U, D, complex_input=True)
    assert plan.route == ref.route(K, U, D) == 2 and plan.period_out == 65536 and plan.period_in == 65535
    assert {k for _, _, k in ref.phases(K, U, D)} == {3, 4}
    want = ref.upfirdn(xh, taps, U, D)
    assert len(want) == plan.nout(n) > 65536 + 256
    got = plan(gpu.from_numpy(xh).cuda())
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_route_2_at_the_largest_decimation(gpu, redio, oracle):
    """U = 65536 against D = 2^31 - 1, 2^20 + 1 taps: consecutive outputs start 32768 samples apart, the first 512 reach to sample
    2^24 -- s(r) near the top of what the phase table's int holds at this input, from r D in 64 bits"""
    U, D, K = 65536, 2 ** 31 - 1, 2 ** 20 + 1
    n = ref.n_for(512, K, U, D)
    assert 2 ** 24 - 32768 < n <= 2 ** 24 + 17 and ref.nout(n, K, U, D) == 512
    taps, xh = oracle.synth_f32(3, K, K), oracle.synth_f32(SEED, 1, n)
    plan = redio.Upfirdn(taps, U, D, fused=True)
    assert plan.route == ref.route(K, U, D) == 2 and plan.period_out == 65536 and plan.period_in == D and plan.nout(n) == 512
    table = ref.phases(K, U, D)
    assert max(s + k for _, s, k in table[:512]) == n and {k for _, _, k in table} == {16, 17}
    want = ref.upfirdn(xh, taps, U, D, True)
    got = plan(gpu.from_numpy(xh).cuda())
    assert got.numel() == 512 and np.array_equal(bits(got.cpu().numpy()), bits(want))


def test_route_2_at_the_most_taps(gpu, redio, oracle):
    """2^24 taps, create's limit, up by 65536: 256 taps per phase, 4 x 65536 + 1 outputs from 260 samples"""
    U, D, K, n = 65536, 1, 2 ** 24, 260
    taps, xh = oracle.synth_f32(3, 1, K), oracle.synth_iq(SEED, 2, n)
    plan = redio.Upfirdn(taps, U, D, complex_input=True)
    assert plan.route == ref.route(K, U, D) == 2 and plan.window == ref.window(K, U, D) == 257  # a period: 65536 outputs over 257 samples
    assert {k for _, _, k in ref.phases(K, U, D)} == {256}
    want = ref.upfirdn(xh, taps, U, D)
    assert len(want) == plan.nout(n) == 4 * 65536 + 1
    got = plan(gpu.from_numpy(xh).cuda())
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    # one plan above each of create's limits (U = 65537, D = 2^31, K = 2^24 + 1) is refused in test_gpu_upfirdn_misuse.py
