"""The synthesis filterbank (redio_pfb_synth_*) on the device, bit for bit against the oracle restatement (tests/pfb_synth_ref.py):
the 64-channel wave kernel (route 1), the same plans sent down the two-pass route, and the two-pass route's own shapes."""
import functools

import numpy as np
import pytest

import pfb_synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED5177
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.5, 2.0 ** -126, -(2.0 ** -126), 2.0 ** 127], np.float32)  # the ladder of test_gpu_ddc.py
# output rows of the route-1 cases: none, one, around a tile (16), around a wave's smallest run (64), past one workgroup of 4 x 64, and 529
ROWS = [0, 1, 15, 16, 17, 63, 64, 65, 257, 529]
BOUND = 2e-6  # relative L2 of a transform against float64


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


@functools.lru_cache(maxsize=None)
def case(M, P, fused, rows):
    """input rows, prototype and the ref's output for `rows` output rows -- computed once, shared, never written to"""
    import oracle
    x = oracle.synth_iq(SEED, 64 * M + P, (rows + P - 1) * M)
    h = oracle.synth_f32(3, M * P, M * P)
    want = ref.synth(x, h, M, P, fused)
    for a in (x, h, want):
        a.setflags(write=False)
    return x, h, want


def put(gpu, a, off):
    """the values on the device at a 16-byte aligned address (off = 0) or one 8 bytes past it (off = 1)"""
    buf = gpu.zeros(len(a) + 2, dtype=gpu.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + len(a)]
    v.copy_(gpu.from_numpy(np.array(a)))
    return v


def run_all_lengths(gpu, plan, M, P, fused, rows_list, want_route):
    x, h, want = case(M, P, fused, max(rows_list))
    ins = {off: put(gpu, x, off) for off in (0, 1)}
    obuf = gpu.empty(len(want) + 2, dtype=gpu.complex64, device="cuda")
    assert plan.route == want_route == int(plan.is_fused)
    for rows in rows_list:
        n_in = (rows + P - 1) * M
        assert plan.nout(n_in) == ref.nout(n_in, M, P) == rows * M
        assert plan.nout(n_in + M - 1) == rows * M  # a trailing partial row is ignored
        for off in (0, 1):
            for ooff in (0, 1):
                obuf.fill_(7.0)
                got = plan(ins[off][:n_in], out=obuf[ooff:])
                assert got.numel() == rows * M
                assert np.array_equal(bits(got.cpu().numpy()), bits(want[: rows * M])), (rows, off, ooff)
                assert (obuf[ooff + rows * M:] == 7.0).all().item(), "wrote past the output"


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_wave_kernel_against_the_ref(gpu, redio, P, fused):
    _, h, _ = case(64, P, fused, max(ROWS))
    plan = redio.Synthesizer(h, 64, P, fused=fused)
    assert ref.route(64, P) == 1
    run_all_lengths(gpu, plan, 64, P, fused, ROWS, 1)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_the_same_plans_unfused_give_the_same_bits(gpu, redio, P, fused):
    x, h, want = case(64, P, fused, max(ROWS))
    plan = redio.Synthesizer(h, 64, P, fused=fused)
    xd = put(gpu, x, 0)
    one = plan(xd).cpu().numpy()
    plan.set_unfused(True)
    run_all_lengths(gpu, plan, 64, P, fused, ROWS, 0)
    two = plan(xd).cpu().numpy()
    assert np.array_equal(bits(one), bits(two)) and np.array_equal(bits(two), bits(want))
    plan.set_unfused(False)
    assert plan.route == 1


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", [(32, 8), (12, 3), (256, 4), (64, 5), (100, 2)])
def test_two_pass_shapes(gpu, redio, M, P, fused):
    _, h, _ = case(M, P, fused, 40)
    plan = redio.Synthesizer(h, M, P, fused=fused)
    assert ref.route(M, P) == 0
    run_all_lengths(gpu, plan, M, P, fused, [0, 1, 40], 0)


@pytest.mark.parametrize("M,P", [(32, 8), (64, 16)])
def test_two_pass_across_scratch_chunk_edges(gpu, redio, M, P):
    """The chunk size is lowered through redio_pfb_synth_set_chunk_rows (64 MiB of rows would take 2^23 values per pass): passes of
    P + 4 input rows = 5 output rows, whose edges overlap by P - 1 rows; 43 rows end on a short pass.  The same bits."""
    x, h, want = case(M, P, True, 43)
    plan = redio.Synthesizer(h, M, P, fused=True)
    plan.set_unfused(True)
    plan.set_chunk_rows(P + 4)
    got = plan(put(gpu, x, 0)).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    plan.set_chunk_rows(1)  # fewer than P counts as P: one output row per pass
    got = plan(put(gpu, x, 1)).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))
    plan.set_chunk_rows(0)  # the default again
    assert np.array_equal(bits(plan(put(gpu, x, 0)).cpu().numpy()), bits(want))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", [(64, 4), (64, 16), (32, 8)])
def test_special_values_in_the_rows(gpu, redio, oracle, M, P, fused):
    rng = np.random.default_rng(SEED + M + P)
    rows = 83
    x, h, _ = case(M, P, fused, rows)
    x, h = x.copy(), h.copy()
    for a, density in ((x, 0.002), (h, 0.03)):
        f = a.view(np.float32).reshape(-1)
        k = max(1, int(density * len(f)))
        f[rng.integers(0, len(f), k)] = SPECIALS[rng.integers(0, len(SPECIALS), k)]
    want = ref.synth(x, h, M, P, fused)
    assert np.isnan(want.view(np.float32)).any() and np.isfinite(want.view(np.float32)).any()
    plan = redio.Synthesizer(h, M, P, fused=fused)
    xd = put(gpu, x, 0)
    assert same_special(plan(xd).cpu().numpy(), want)
    if plan.route == 1:
        plan.set_unfused(True)
        assert same_special(plan(xd).cpu().numpy(), want)


@pytest.mark.parametrize("M,P", [(64, 4), (64, 16), (32, 8)])
def test_channelizer_then_synthesizer(gpu, redio, oracle, M, P):
    n = (3 * P + 70) * M
    xh = oracle.synth_iq(SEED, 11, n)
    ha, hs = oracle.synth_f32(3, 5, M * P), oracle.synth_f32(3, 9, M * P)
    x = gpu.from_numpy(xh).cuda()
    rows = redio.Channelizer(ha, M, P, fused=True)(x)
    got = redio.Synthesizer(hs, M, P, fused=True)(rows.reshape(-1)).cpu().numpy()
    want = ref.synth(oracle.pfb_channelizer(xh, ha, M, P, True).reshape(-1), hs, M, P, True)
    assert len(want) > 0 and np.array_equal(bits(got), bits(want))
    # one-tap prototypes: a 1.0 at tap pa of every analysis branch, at ps of every synthesis branch -> M x, delayed by (pa + ps) M
    pa, ps = 1, P - 2
    ea, es = np.zeros(M * P, np.float32), np.zeros(M * P, np.float32)
    ea[pa * M: (pa + 1) * M] = 1.0
    es[ps * M: (ps + 1) * M] = 1.0
    got = redio.Synthesizer(es, M, P, fused=True)(redio.Channelizer(ea, M, P, fused=True)(x).reshape(-1)).cpu().numpy()
    d = (pa + ps) * M
    want = M * xh[d: d + len(got)].astype(np.complex128)
    assert len(got) == n - 2 * (P - 1) * M
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print(f"one-tap round trip {M}x{P}: relative L2 {err:.3e}")
    assert err <= BOUND


def test_seeded_random_cases(gpu, redio, oracle):
    rng = np.random.default_rng(SEED)
    shapes = [(64, 4), (64, 8), (64, 16), (64, 16), (32, 8), (12, 3), (256, 4), (64, 5), (100, 2), (7, 1)]
    for i in range(20):
        M, P = shapes[int(rng.integers(0, len(shapes)))]
        fused = bool(rng.integers(0, 2))
        rows = int(rng.integers(0, 300 if M <= 64 else 40))
        extra = int(rng.integers(0, M))  # a trailing partial row
        off, ooff = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        x = oracle.synth_iq(SEED + i, i, (rows + P - 1) * M + extra)
        h = oracle.synth_f32(3 + i, M, M * P)
        want = ref.synth(x, h, M, P, fused)
        plan = redio.Synthesizer(h, M, P, fused=fused)
        unf = bool(rng.integers(0, 2))
        if unf:
            plan.set_unfused(True)
        assert plan.route == (0 if unf else ref.route(M, P))
        obuf = gpu.empty(len(want) + 2, dtype=gpu.complex64, device="cuda")
        got = plan(put(gpu, x, off), out=obuf[ooff:])
        assert got.numel() == len(want) == ref.nout(len(x), M, P)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (i, M, P, fused, rows, extra, off, ooff, unf)
