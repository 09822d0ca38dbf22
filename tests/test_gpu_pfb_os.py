"""The oversampled channelizer (redio_pfb_os_*) on the device, bit for bit against the oracle restatement (tests/pfb_os_ref.py): the
64-channel wave kernel at hop 32 (route 1), the same plans sent down the two-pass route, the two-pass route's own shapes, its chunk
seams, hop = nchan against the Channelizer, special values, and one launch above the geometry's floor."""
import functools

import numpy as np
import pytest

import pfb_os_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0533
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan,
                     1.0, -1.0, 0.5, 2.0 ** -126, -(2.0 ** -126), 2.0 ** 127], np.float32)  # the ladder of test_gpu_pfb_synth.py
# rows of the route-1 cases: none, one, around a tile (16), around a wave's smallest run (64), past one workgroup of 4 x 64, and 529
ROWS = [0, 1, 15, 16, 17, 63, 64, 65, 257, 529]
FIRST = [0, 1, 2 ** 64 - 530]


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


def n_in(M, P, H, rows):
    return M * P + H * (rows - 1) if rows else M * P - 1


@functools.lru_cache(maxsize=None)
def case(M, P, H, fused, rows):
    """input, prototype and the ref's branch sums for `rows` rows -- computed once, shared, never written to"""
    import oracle
    x = oracle.synth_iq(SEED, 64 * M + P, n_in(M, P, H, rows) + H - 1)  # H - 1 samples behind the last row's window: never read
    h = oracle.synth_f32(3, M * P, M * P)
    u = ref.branch_sums(x, h, M, P, H, fused)
    for a in (x, h, u):
        a.setflags(write=False)
    return x, h, u


@functools.lru_cache(maxsize=None)
def want_rows(M, P, H, fused, rows, F):
    """the ref's rows for first_row = F; row r of a shorter call on a prefix of the input is row r of this one"""
    import oracle
    _, _, u = case(M, P, H, fused, rows)
    w = oracle.fft(np.ascontiguousarray(ref.roll_rows(u, M, H, F).reshape(-1)), M, inverse=False).reshape(-1, M)
    w.setflags(write=False)
    return w


def put(gpu, a, off):
    """the values on the device at a 16-byte aligned address (off = 0) or one 8 bytes past it (off = 1)"""
    buf = gpu.zeros(len(a) + 2, dtype=gpu.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + len(a)]
    v.copy_(gpu.from_numpy(np.array(a)))
    return v


def run_all_lengths(gpu, plan, M, P, H, fused, rows_list, firsts, want_route):
    top = max(rows_list)
    x, h, _ = case(M, P, H, fused, top)
    ins = {off: put(gpu, x, off) for off in (0, 1)}
    obuf = gpu.empty(top * M + 2, dtype=gpu.complex64, device="cuda")
    assert plan.route == want_route == int(plan.is_fused) and plan.hop == H
    for rows in rows_list:
        n = n_in(M, P, H, rows)
        assert plan.nrows(n) == ref.nrows(n, M, P, H) == rows
        extra = H - 1 if rows else 0  # samples short of one more row are not read
        assert plan.nrows(n + extra) == rows
        for F in firsts:
            want = want_rows(M, P, H, fused, top, F)[:rows]
            for off, ooff in ((0, 0), (1, 0), (0, 1), (1, 1)):
                obuf.fill_(7.0)
                got = plan(ins[off][: n + extra], first_row=F, out=obuf[ooff:])
                assert got.shape == (rows, M)
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (rows, F, off, ooff)
                assert (obuf[ooff + rows * M:] == 7.0).all().item() and (obuf[:ooff] == 7.0).all().item(), "wrote outside the output"


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_wave_kernel_against_the_ref(gpu, redio, P, fused):
    _, h, _ = case(64, P, 32, fused, max(ROWS))
    plan = redio.OversampledChannelizer(h, 64, P, 32, fused=fused)
    assert ref.route(64, P, 32) == 1
    run_all_lengths(gpu, plan, 64, P, 32, fused, ROWS, FIRST, 1)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_the_same_plans_unfused_give_the_same_bits(gpu, redio, P, fused):
    x, h, _ = case(64, P, 32, fused, max(ROWS))
    plan = redio.OversampledChannelizer(h, 64, P, 32, fused=fused)
    xd = put(gpu, x, 0)
    one = plan(xd, first_row=1).cpu().numpy()
    plan.set_unfused(True)
    run_all_lengths(gpu, plan, 64, P, 32, fused, ROWS, FIRST, 0)
    two = plan(xd, first_row=1).cpu().numpy()
    assert np.array_equal(bits(one), bits(two)) and np.array_equal(bits(two), bits(want_rows(64, P, 32, fused, max(ROWS), 1)))
    plan.set_unfused(False)
    assert plan.route == 1


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P,H", [(64, 16, 16), (64, 5, 32), (64, 8, 48), (32, 8, 16), (256, 4, 128), (12, 3, 5), (100, 2, 100)])
def test_two_pass_shapes(gpu, redio, M, P, H, fused):
    _, h, _ = case(M, P, H, fused, 40)
    plan = redio.OversampledChannelizer(h, M, P, H, fused=fused)
    assert ref.route(M, P, H) == 0
    run_all_lengths(gpu, plan, M, P, H, fused, [0, 1, 40], [0, 1, 3, 2 ** 64 - 41], 0)


@pytest.mark.parametrize("M,P,H", [(64, 16, 32), (64, 8, 48), (12, 3, 5)])
def test_two_pass_across_scratch_chunk_edges(gpu, redio, M, P, H):
    """The chunk size is lowered through redio_pfb_os_set_chunk_rows (64 MiB of rows would take 2^23 values per pass): 5 rows per
    pass over 43 rows, which end on a short pass; the shift goes on across the seams.  The same bits."""
    x, h, _ = case(M, P, H, True, 43)
    plan = redio.OversampledChannelizer(h, M, P, H, fused=True)
    plan.set_unfused(True)
    xd = put(gpu, x, 1)
    for F in (0, 3):
        want = want_rows(M, P, H, True, 43, F)
        plan.set_chunk_rows(5)
        assert np.array_equal(bits(plan(xd, first_row=F).cpu().numpy()), bits(want))
        plan.set_chunk_rows(1)
        assert np.array_equal(bits(plan(xd, first_row=F).cpu().numpy()), bits(want))
        plan.set_chunk_rows(0)  # the default again
        assert np.array_equal(bits(plan(xd, first_row=F).cpu().numpy()), bits(want))


@pytest.mark.parametrize("M,P", [(64, 16), (64, 4), (32, 8), (100, 2)])
def test_at_hop_nchan_the_rows_are_the_channelizers(gpu, redio, oracle, M, P):
    x = oracle.synth_iq(SEED, M, (P + 70) * M + 9)
    h = oracle.synth_f32(3, P, M * P)
    xd = gpu.from_numpy(x).cuda()
    for fused in (False, True):
        want = redio.Channelizer(h, M, P, fused=fused)(xd).cpu().numpy().reshape(-1, M)
        plan = redio.OversampledChannelizer(h, M, P, M, fused=fused)
        assert plan.route == 0 and plan.nrows(len(x)) == 71
        for F in (0, 5):
            assert np.array_equal(bits(plan(xd, first_row=F).cpu().numpy()), bits(want))
        assert np.array_equal(bits(want), bits(oracle.pfb_channelizer(x, h, M, P, fused)))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P,H", [(64, 4, 32), (64, 16, 32), (64, 16, 16), (32, 8, 16)])
def test_special_values_in_the_stream(gpu, redio, oracle, M, P, H, fused):
    """The whole ladder, every value twice, in the first fifth of the stream: a row's transform spreads one NaN or infinity over all its
    channels, and every sample lies in nchan * taps_per_branch / hop windows, so values all over the stream would leave no finite row
    (the synthesis bank filters behind its transform, where a value stays in its column).  For the same reason the prototype gets the
    ladder's members up to 2.0 in magnitude only: a tap is in every row."""
    rng = np.random.default_rng(SEED + M + P + H)
    x, h, _ = case(M, P, H, fused, 83)
    x, h = x.copy(), h.copy()
    f = x.view(np.float32).reshape(-1)
    f[rng.choice(len(f) // 5, 2 * len(SPECIALS), replace=False)] = np.tile(SPECIALS, 2)
    mild = SPECIALS[np.abs(SPECIALS) <= 2.0]
    k = max(1, int(0.03 * len(h)))
    h[rng.integers(0, len(h), k)] = mild[rng.integers(0, len(mild), k)]
    want = ref.channelize(x, h, M, P, H, 1, fused)
    assert np.isnan(want.view(np.float32)).any() and np.isfinite(want.view(np.float32)).any()
    plan = redio.OversampledChannelizer(h, M, P, H, fused=fused)
    xd = put(gpu, x, 0)
    assert plan.route == ref.route(M, P, H)
    assert same_special(plan(xd, first_row=1).cpu().numpy(), want)
    if plan.route == 1:
        plan.set_unfused(True)
        assert same_special(plan(xd, first_row=1).cpu().numpy(), want)


def test_launch_above_the_geometry_floor(gpu, redio, oracle):
    """2048 * 64 + 17 rows: runs of 80 rows (five tiles: an odd count, the pair loop's single-tile end) over 1639 wavefronts, the
    last one cut; every row compared."""
    M, P, H, rows = 64, 4, 32, 2048 * 64 + 17
    assert ref.rows_per_wave(rows) == 80 and ref.waves(rows) == 1639
    x = oracle.synth_iq(SEED, 5, n_in(M, P, H, rows))
    h = oracle.synth_f32(3, 5, M * P)
    want = ref.channelize(x, h, M, P, H, 1, True)
    plan = redio.OversampledChannelizer(h, M, P, H, fused=True)
    out = gpu.full((rows * M + 2,), 7.0, dtype=gpu.complex64, device="cuda")
    got = plan(gpu.from_numpy(x).cuda(), first_row=1, out=out)
    assert got.shape == want.shape == (rows, M)
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert (out[rows * M:] == 7.0).all().item()
