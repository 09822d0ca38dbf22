"""The launch geometry of the polyphase spectrometer's workgroup kernel (route 2).  pfbspec_p2_units_per_stream
(libredio_amd/csrc/pfb_pspec_p2_core.h) gives a stream max(ceil(nunits / (4 CUs G)), least) consecutive units -- output rows, or by
segments segments -- with G = max(1, 256 / M) streams per workgroup and least = ceil(64 / K) rows or 4 segments.  On the floor:
several workgroups and a short last stream at 32 x 4 (eight streams per workgroup), 256 x 8 and 1024 x 4, by segments with K = 17
and K = 40 so that the streams of one workgroup differ in phase and in iteration count, against the restatement on the CPU.  Above
the floor: about 20 M samples at 32 x 4 by rows and by segments, against the unflagged plan on the GPU (which the other tests hold to
the restatement).  Auto mode one output row either side of its threshold of 2 CUs G ceil(64 / K) rows.  The figures are asserted from
a restatement of the launcher's arithmetic with the device's CU count."""
import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F61
SEG = 16  # PSPEC_SEG
AUTO, ROWS, SEGMENTS = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cus(gpu):
    return gpu.cuda.get_device_properties(0).multi_processor_count


def streams_per_group(M):
    return max(1, 256 // M)


def units_per_stream(nunits, K, split, ncus, M):
    """pfbspec_p2_units_per_stream: (units a stream owns, its floor)"""
    least = -(-64 // (SEG if split else K))
    return max(-(-nunits // (4 * ncus * streams_per_group(M))), least), least


def split_rows(K, ncus, M):
    """pfbspec_p2_split_rows: auto mode is rows mode from this many output rows"""
    return 2 * ncus * streams_per_group(M) * -(-64 // K)


def geometry(mode, K, rows, ncus, M):
    """(split, units, units per stream, floor, workgroups) of a call of `rows` output rows on a route-2 plan"""
    S = -(-K // SEG)
    split = S >= 2 and (mode == SEGMENTS or (mode == AUTO and rows < split_rows(K, ncus, M)))
    units = rows * S if split else rows
    ups, least = units_per_stream(units, K, split, ncus, M)
    return split, units, ups, least, -(-(-(-units // ups)) // streams_per_group(M))


# M, P, K, output rows, mode, from bytes: a few hundred thousand samples
FLOOR = [
    (32, 4, 17, 401, ROWS, False), (32, 4, 17, 401, SEGMENTS, False), (32, 4, 17, 401, SEGMENTS, True), (32, 4, 40, 171, SEGMENTS, False),
    (256, 8, 17, 69, ROWS, False), (256, 8, 17, 69, SEGMENTS, True), (256, 8, 40, 29, SEGMENTS, False),
    (1024, 4, 40, 7, ROWS, True), (1024, 4, 17, 19, SEGMENTS, False), (1024, 4, 40, 7, SEGMENTS, False),
]


@pytest.mark.parametrize("M,P,K,rows,mode,u8", FLOOR)
def test_on_the_floor(gpu, redio, oracle, M, P, K, rows, mode, u8):
    split, units, ups, least, groups = geometry(mode, K, rows, cus(gpu), M)
    assert split == (mode == SEGMENTS) and ups == least, "this shape no longer sits on the launcher's floor"
    assert groups >= 3 and units % ups, "no longer several workgroups with a short last stream"
    n = M * (rows * K + P - 1) + M * (K - 1) + 3
    assert 200_000 <= n < 400_000
    h = oracle.synth_f32(9, P, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK and plan.nrows(n) == rows
    plan.set_split(mode)
    out = gpu.full((rows * M + M,), float("nan"), dtype=gpu.float32, device="cuda")
    if u8:
        raw = np.random.default_rng(SEED + K).integers(0, 256, 2 * n, dtype=np.uint8)
        got, want = plan.from_bytes(gpu.from_numpy(raw).cuda(), out=out), ref.spectrum_u8(raw, h, M, P, K, True)
    else:
        x = oracle.synth_iq(SEED, K, n)
        got, want = plan(gpu.from_numpy(x).cuda(), out=out), ref.spectrum(x, h, M, P, K, True)
    got = got.cpu().numpy()
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert got.shape == want.shape == (rows, M) and not len(bad), (len(bad), bad[:8])
    assert bool(out[rows * M:].isnan().all())


@pytest.mark.parametrize("mode", [ROWS, SEGMENTS])
def test_above_the_floor(gpu, redio, oracle, mode):
    """32 x 4, K = 17: nine eighths of the rows the floor covers, about 20 M samples on 256 CUs.  A stream owns more units than the
    floor, the last stream is short, and by segments (S = 2) a run of an odd number of segments starts in the middle of a row."""
    M, P, K = 32, 4, 17
    ncus = cus(gpu)
    rows = 4 * ncus * streams_per_group(M) * 4 * 9 // 8 - 3
    split, units, ups, least, _ = geometry(mode, K, rows, ncus, M)
    assert split == (mode == SEGMENTS) and ups > least, "this shape no longer runs above the launcher's floor"
    assert units % ups, "the last stream is no longer a short one"
    if split:
        assert ups % 2, "no stream starts in the middle of an output row any more"
    n = M * (rows * K + P - 1) + M * (K - 1) + 3
    h = oracle.synth_f32(9, P, M * P)
    x = redio.synth_iq(SEED, K, n)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    base = redio.PolyphaseSpectrum(h, M, P, K)
    assert plan.route == plan.BLOCK and base.route == base.GENERIC and plan.nrows(n) == rows
    plan.set_split(mode)
    out = gpu.full((rows * M + M,), float("nan"), dtype=gpu.float32, device="cuda")
    got, want = plan(x, out=out), base(x)
    assert got.shape == want.shape == (rows, M) and not bool(want.isnan().any())
    assert gpu.equal(got.view(gpu.int32), want.view(gpu.int32))
    assert bool(out[rows * M:].isnan().all())


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("side", [-1, 0])
def test_auto_either_side_of_its_threshold(gpu, redio, oracle, side, u8):
    """32 x 4, K = 17: auto mode works by segments below 2 * CUs * 8 * 4 output rows and by rows from there on.  By segments the call
    sizes the plan's partials -- the one allocation such a call makes -- and by rows it allocates nothing."""
    M, P, K = 32, 4, 17
    ncus = cus(gpu)
    edge = split_rows(K, ncus, M)
    assert edge == 2 * ncus * 8 * 4
    rows = edge + side
    assert geometry(AUTO, K, rows, ncus, M)[0] == (side < 0)
    n = M * (rows * K + P - 1) + 5
    h = oracle.synth_f32(9, P, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    base = redio.PolyphaseSpectrum(h, M, P, K)
    assert plan.route == plan.BLOCK and plan.nrows(n) == rows
    if u8:
        d = gpu.from_numpy(np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8)).cuda()
        want = base.from_bytes(d)
    else:
        d = redio.synth_iq(SEED, 3, n)
        want = base(d)
    out = gpu.full((rows * M + M,), float("nan"), dtype=gpu.float32, device="cuda")
    count = redio.lib().redio_malloc_count()
    got = (plan.from_bytes if u8 else plan)(d, out=out)
    assert redio.lib().redio_malloc_count() - count == (1 if side < 0 else 0)
    assert gpu.equal(got.view(gpu.int32), want.view(gpu.int32)) and bool(out[rows * M:].isnan().all())
