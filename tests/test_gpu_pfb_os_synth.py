"""The oversampled synthesis bank (redio_pfb_os_synth_*) on the device, bit for bit against the oracle restatement
(tests/pfb_os_synth_ref.py): the 64-channel wave kernel at hop 32 (route 1), the same plans sent down the two-pass route, the two-pass
route's own shapes and its chunk seams, hop = nchan against the Synthesizer, the round trip through the OversampledChannelizer, special
values, and one launch above the geometry's floor.  Rows in are hops out plus L - 1."""
import functools

import numpy as np
import pytest

import pfb_os_ref
import pfb_os_synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0534
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.5, 2.0 ** -126, -(2.0 ** -126), 2.0 ** 127], np.float32)  # the ladder of test_gpu_pfb_synth.py
# hops of the route-1 cases: none, one, around a tile (16), around a wave's smallest run (64), past one workgroup of 4 x 64, and 529
HOPS = [0, 1, 15, 16, 17, 63, 64, 65, 257, 529]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_special(got, want):
    """bit for bit, NaNs by position (as test_gpu_pfb_synth.py)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


def firsts(T):
    return [0, 1, 2 ** 64 - 1 - T]


@functools.lru_cache(maxsize=None)
def case(M, P, H, hops):
    """channel values for `hops` hops, the prototype and the rows behind the inverse transform -- computed once, shared, never written to"""
    import oracle
    L = ref.nrows_per_hop(M, P, H)
    X = oracle.synth_iq(SEED, 64 * M + P, (hops + L - 1) * M + M - 1)  # a trailing partial row: ignored
    h = oracle.synth_f32(3, M * P, M * P)
    W = ref.inverse_rows(X, M)
    for a in (X, h, W):
        a.setflags(write=False)
    return X, h, W


@functools.lru_cache(maxsize=None)
def want_out(M, P, H, fused, hops, Fm):
    """the ref's samples for first_row = Fm (mod M: all the column depends on); hop q of a shorter call on a prefix of the rows is hop q
    of this one"""
    _, h, W = case(M, P, H, hops)
    y = ref.overlap_add(W, h, M, P, H, Fm, fused)
    y.setflags(write=False)
    return y


def put(gpu, a, off):
    """the values on the device at a 16-byte aligned address (off = 0) or one 8 bytes past it (off = 1)"""
    buf = gpu.zeros(len(a) + 2, dtype=gpu.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + len(a)]
    v.copy_(gpu.from_numpy(np.array(a)))
    return v


def run_all_lengths(gpu, plan, M, P, H, fused, hops_list, want_route, offs=((0, 0), (1, 0), (0, 1), (1, 1))):
    top = max(hops_list)
    L = ref.nrows_per_hop(M, P, H)
    X, h, _ = case(M, P, H, top)
    ins = {off: put(gpu, X, off) for off in (0, 1)}
    obuf = gpu.empty(top * H + 2, dtype=gpu.complex64, device="cuda")
    assert plan.route == want_route == int(plan.is_fused) and plan.hop == H
    for hops in hops_list:
        T = hops + L - 1
        n = T * M
        assert plan.nout(n) == ref.nout(n, M, P, H) == hops * H
        extra = M - 1  # a trailing partial row is ignored
        assert plan.nout(n + extra) == hops * H
        for F in firsts(T):
            want = want_out(M, P, H, fused, top, F % M)[: hops * H]
            for off, ooff in offs:
                obuf.fill_(7.0)
                got = plan(ins[off][: n + extra], first_row=F, out=obuf[ooff:])
                assert got.shape == (hops * H,)
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (hops, F, off, ooff)
                assert (obuf[ooff + hops * H:] == 7.0).all().item() and (obuf[:ooff] == 7.0).all().item(), "wrote outside the output"


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_wave_kernel_against_the_ref(gpu, redio, P, fused):
    _, h, _ = case(64, P, 32, max(HOPS))
    plan = redio.OversampledSynthesizer(h, 64, P, 32, fused=fused)
    assert ref.route(64, P, 32) == 1
    run_all_lengths(gpu, plan, 64, P, 32, fused, HOPS, 1)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_the_same_plans_unfused_give_the_same_bits(gpu, redio, P, fused):
    X, h, _ = case(64, P, 32, max(HOPS))
    plan = redio.OversampledSynthesizer(h, 64, P, 32, fused=fused)
    Xd = put(gpu, X, 1)
    one = plan(Xd, first_row=1).cpu().numpy()
    plan.set_unfused(True)
    run_all_lengths(gpu, plan, 64, P, 32, fused, HOPS, 0, offs=((1, 1),))
    two = plan(Xd, first_row=1).cpu().numpy()
    assert np.array_equal(bits(one), bits(two)) and np.array_equal(bits(two), bits(want_out(64, P, 32, fused, max(HOPS), 1)))
    plan.set_unfused(False)
    assert plan.route == 1


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P,H", [(64, 4, 16), (64, 4, 48), (64, 4, 64), (32, 3, 20), (12, 2, 5), (256, 8, 128)])
def test_two_pass_shapes(gpu, redio, M, P, H, fused):
    """route 0 against the ref, whole and with the chunk set to L and L + 1 input rows (one and two hops per pass): the seams"""
    _, h, _ = case(M, P, H, 40)
    plan = redio.OversampledSynthesizer(h, M, P, H, fused=fused)
    assert ref.route(M, P, H) == 0
    L = ref.nrows_per_hop(M, P, H)
    for chunk in (0, L, L + 1):
        plan.set_chunk_rows(chunk)
        run_all_lengths(gpu, plan, M, P, H, fused, [0, 1, 40], 0, offs=((0, 0), (1, 1)))


@pytest.mark.parametrize("P", [4, 16])
def test_route_1_plans_across_scratch_chunk_edges(gpu, redio, P):
    """a route-1 plan sent down route 0 in passes of L, L + 1 and L + 4 rows: the wave kernel's bits at every seam"""
    X, h, _ = case(64, P, 32, 65)
    plan = redio.OversampledSynthesizer(h, 64, P, 32, fused=True)
    Xd = put(gpu, X, 1)
    L = 2 * P
    for F in (0, 3):
        plan.set_unfused(False)
        one = plan(Xd, first_row=F).cpu().numpy()
        assert np.array_equal(bits(one), bits(want_out(64, P, 32, True, 65, F)))
        plan.set_unfused(True)
        for chunk in (L, L + 1, L + 4, 0):
            plan.set_chunk_rows(chunk)
            assert np.array_equal(bits(plan(Xd, first_row=F).cpu().numpy()), bits(one)), (F, chunk)


@pytest.mark.parametrize("M,P", [(64, 16), (64, 4), (32, 8), (100, 2)])
def test_at_hop_nchan_the_output_is_the_synthesizers(gpu, redio, oracle, M, P):
    X = oracle.synth_iq(SEED, M, (P + 70) * M + 9)
    h = oracle.synth_f32(3, P, M * P)
    Xd = gpu.from_numpy(X).cuda()
    for fused in (False, True):
        want = redio.Synthesizer(h, M, P, fused=fused)(Xd).cpu().numpy().reshape(-1)
        plan = redio.OversampledSynthesizer(h, M, P, M, fused=fused)
        assert plan.route == 0 and plan.nout(len(X)) == 71 * M == len(want)
        for F in (0, 5):
            assert np.array_equal(bits(plan(Xd, first_row=F).cpu().numpy()), bits(want))


def windows(M, P, H):
    """test_pfb_os_synth_cpu.windows: analysis and synthesis prototypes on window positions [0, M) that overlap-add to one"""
    i = np.arange(M)
    if 2 * H == M:
        a = np.sin(np.pi * (i + 0.5) / M)
    else:
        ov = M - H
        a = np.sqrt(np.where(i < ov, (i + 0.5) / ov, np.where(i < H, 1.0, 1.0 - (i - H + 0.5) / ov)))
    ha, hs = np.zeros(M * P, np.float32), np.zeros(M * P, np.float32)
    ha[:M] = a
    hs[[ref.tap(o, M, P) for o in range(M)]] = a
    return ha, hs


@pytest.mark.parametrize("M,P,H", [(64, 4, 32), (64, 4, 48), (12, 2, 7)])
def test_device_round_trip_is_the_refs(gpu, redio, oracle, M, P, H):
    """OversampledChannelizer into OversampledSynthesizer on the device: the bits of the reference round trip, and M x[(L - 1) H + n]
    within two transforms' rounding (test_pfb_os_synth_cpu.py: 4e-6)"""
    T = 75
    L = ref.nrows_per_hop(M, P, H)
    x = oracle.synth_iq(SEED, H, M * P + (T - 1) * H)
    ha, hs = windows(M, P, H)
    xd = put(gpu, x, 0)
    for F in (0, 5):
        rows = redio.OversampledChannelizer(ha, M, P, H, fused=False)(xd, first_row=F)
        assert rows.shape == (T, M)
        y = redio.OversampledSynthesizer(hs, M, P, H, fused=False)(rows.reshape(-1), first_row=F).cpu().numpy()
        want = ref.synth(pfb_os_ref.channelize(x, ha, M, P, H, F).reshape(-1), hs, M, P, H, F)
        assert np.array_equal(bits(y), bits(want))
        exact = M * x[(L - 1) * H: (L - 1) * H + len(y)].astype(np.complex128)
        assert len(y) == (T - L + 1) * H and np.linalg.norm(y - exact) / np.linalg.norm(exact) <= 4e-6


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P,H", [(64, 4, 32), (64, 16, 32), (64, 4, 48), (32, 3, 20)])
def test_special_values_among_the_channel_values(gpu, redio, oracle, M, P, H, fused):
    """Signed zeros, subnormals, infinities and NaN, every value twice, in the first fifth of the rows (a row's transform spreads one NaN
    or infinity over the whole row, and a row is in L hops); the prototype gets the ladder's members up to 2.0 in magnitude."""
    rng = np.random.default_rng(SEED + M + P + H)
    X, h, _ = case(M, P, H, 83)
    X, h = X.copy(), h.copy()
    f = X.view(np.float32).reshape(-1)
    f[rng.choice(len(f) // 5, 2 * len(SPECIALS), replace=False)] = np.tile(SPECIALS, 2)
    mild = SPECIALS[np.abs(SPECIALS) <= 2.0]
    k = max(1, int(0.03 * len(h)))
    h[rng.integers(0, len(h), k)] = mild[rng.integers(0, len(mild), k)]
    want = ref.synth(X, h, M, P, H, 1, fused)
    assert np.isnan(want.view(np.float32)).any() and np.isfinite(want.view(np.float32)).any()
    plan = redio.OversampledSynthesizer(h, M, P, H, fused=fused)
    Xd = put(gpu, X, 0)
    assert plan.route == ref.route(M, P, H)
    assert same_special(plan(Xd, first_row=1).cpu().numpy(), want)
    if plan.route == 1:
        plan.set_unfused(True)
        assert same_special(plan(Xd, first_row=1).cpu().numpy(), want)


def test_launch_above_the_geometry_floor(gpu, redio, oracle):
    """2048 * 64 + 17 hops: runs of 80 hops (an odd count of tiles and a halo: the pair loop's single-tile end and both tile parities)
    over 1639 wavefronts, the last one cut; every sample compared."""
    M, P, H, hops = 64, 4, 32, 2048 * 64 + 17
    assert ref.hops_per_wave(hops) == 80 and ref.waves(hops) == 1639
    X = oracle.synth_iq(SEED, 5, (hops + 2 * P - 1) * M)
    h = oracle.synth_f32(3, 5, M * P)
    want = ref.synth(X, h, M, P, H, 1, True)
    plan = redio.OversampledSynthesizer(h, M, P, H, fused=True)
    out = gpu.full((hops * H + 2,), 7.0, dtype=gpu.complex64, device="cuda")
    got = plan(gpu.from_numpy(X).cuda(), first_row=1, out=out)
    assert got.shape == want.shape == (hops * H,)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert (out[hops * H:] == 7.0).all().item()
