"""The one driver of the three two-pass filterbank plans (libredio_amd/csrc/pfb_bank.hip, pfb_bank_cut.h) at its edges, on fixed
shapes, every result bit for bit against the restatements (tests/pfb_synth_ref.py, pfb_os_ref.py, pfb_os_synth_ref.py):

  - the seam of the DEFAULT chunk (64 MiB of rows; no set_chunk_rows): 2048 * 64 + 17 units at 64 channels down route 0, and one call at
    100 channels, where 64 MiB is no whole number of rows.  The cut is restated here, so that the test fails if the default moves;
  - a channel count whose transform stages through a work buffer (8194 = 2 17 241): the fft_stages / fft_cap branch of reserve and
    enqueue, with chunk settings that change the pass from call to call, and under stream capture;
  - degenerate shapes: one channel, one tap per branch, hop 1, prime channel counts, hops coprime to the channel count, 64 channels
    that are not the wave shape -- at 0, 1 and 9 units, first_row 0, 1 and 2^64 - 1 - T, all four in / out alignments."""
import functools
import os
import subprocess

import numpy as np
import pytest

import pfb_os_ref
import pfb_os_synth_ref
import pfb_synth_ref

gpu_test = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0B4C
ERR_NOT_RESERVED = -6
FAMILIES = ["pfb_synth", "pfb_os", "pfb_os_synth"]
LAUNCH_UNITS = 2048 * 64 + 17   # the launch tests' call (test_gpu_pfb_os.py, test_gpu_pfb_os_synth.py, test_gpu_pfb_synth.py)
STAGING = 8194


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cut_of(fam, M, P, H):
    """(window, hop, unit_out, min_rows) of pfb_bank_cut.h's table, restated"""
    if fam == "pfb_synth":
        return M * P, M, M, P
    if fam == "pfb_os":
        return M * P, H, M, 1
    L = -(-M * P // H)
    return M * L, M, H, L


def passes_of(cut, M, asked, units):
    """test_pfb_bank_cut.brute: one unit at a time, a pass of n units holds n + min_rows - 1 rows and takes units while they fit the
    chunk (0: the default, 64 MiB of rows of M cf32; fewer than min_rows count as min_rows) -> [(first unit, units)]"""
    min_rows = cut[3]
    chunk = max(asked if asked else (64 << 20) // (M * 8), min_rows)
    passes, first, n = [], 0, 0
    for u in range(units):
        if n and (n + 1) + min_rows - 1 > chunk:
            passes.append((first, n))
            first, n = u, 0
        n += 1
    passes.append((first, n))
    return passes


def make_plan(redio, fam, h, M, P, H, fused):
    if fam == "pfb_synth":
        return redio.Synthesizer(h, M, P, fused=fused)
    return (redio.OversampledChannelizer if fam == "pfb_os" else redio.OversampledSynthesizer)(h, M, P, H, fused=fused)


def run(plan, fam, dx, F, out=None):
    return (plan(dx, out=out) if fam == "pfb_synth" else plan(dx, first_row=F, out=out)).reshape(-1)


def want_of(fam, x, h, M, P, H, F, fused):
    if fam == "pfb_synth":
        return pfb_synth_ref.synth(x, h, M, P, fused)
    if fam == "pfb_os":
        return pfb_os_ref.channelize(x, h, M, P, H, F, fused).reshape(-1)
    return pfb_os_synth_ref.synth(x, h, M, P, H, F, fused)


@functools.lru_cache(maxsize=None)
def case(fam, M, P, H, units, F, fused, extra=0):
    """input for `units` units (and `extra` elements of a trailing partial), the prototype and the restatement's output -- computed once,
    shared, never written to"""
    import oracle
    window, hop, _, _ = cut_of(fam, M, P, H)
    x = oracle.synth_iq(SEED, M + P + H, (units - 1) * hop + window + extra)
    h = oracle.synth_f32(3, M + P, M * P)
    want = want_of(fam, x, h, M, P, H, F, fused)
    for a in (x, h, want):
        a.setflags(write=False)
    return x, h, want


def put(gpu, a, off):
    """the values on the device at a 16-byte aligned address (off = 0) or one 8 bytes past it (off = 1)"""
    buf = gpu.zeros(len(a) + 2, dtype=gpu.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + len(a)]
    if len(a):
        v.copy_(gpu.from_numpy(np.array(a)))
    return v


# ---- the default chunk's seam --------------------------------------------------------------------------------------------------------------
@gpu_test
@pytest.mark.parametrize("fam", FAMILIES)
def test_default_chunk_seam_on_the_launch_tests_call(gpu, redio, fam):
    """2048 * 64 + 17 units at (64, 4, 32) with set_unfused and the chunk left alone: two passes, the last a short one, the bits of the
    restatement and of the same plan's wave kernel"""
    M, P, H, F, units = 64, 4, 32, 1, LAUNCH_UNITS
    cut = cut_of(fam, M, P, H)
    passes = passes_of(cut, M, 0, units)
    assert len(passes) >= 2 and passes[-1][1] < passes[0][1], passes   # fails if the default chunk moves, instead of going quiet
    assert (64 << 20) // (M * 8) == 131072 and passes[0][1] + cut[3] - 1 == 131072
    x, h, want = case(fam, M, P, H, units, F, True)
    plan = make_plan(redio, fam, h, M, P, H, True)
    dx = gpu.from_numpy(np.array(x)).cuda()
    assert plan.route == 1
    wave = run(plan, fam, dx, F).cpu().numpy()
    plan.set_unfused(True)
    assert plan.route == 0
    out = gpu.full((len(want) + 2,), 7.0, dtype=gpu.complex64, device="cuda")
    got = run(plan, fam, dx, F, out=out[: len(want)]).cpu().numpy()
    assert got.shape == want.shape == (units * cut[2],)
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(wave), bits(want))
    assert (out[len(want):] == 7.0).all().item()


@gpu_test
def test_default_chunk_seam_where_64_mib_is_no_whole_number_of_rows(gpu, redio):
    """100 channels: 83886 rows and 32 bytes over; the oversampled channelizer at (100, 3, 60) across that seam"""
    fam, M, P, H, F = "pfb_os", 100, 3, 60, 3
    assert (64 << 20) // (M * 8) == 83886 and (64 << 20) % (M * 8)
    units = 83886 + 17
    passes = passes_of(cut_of(fam, M, P, H), M, 0, units)
    assert passes == [(0, 83886), (83886, 17)]
    x, h, want = case(fam, M, P, H, units, F, False, extra=H - 1)
    plan = make_plan(redio, fam, h, M, P, H, False)
    assert plan.route == 0 and plan.nrows(len(x)) == units
    got = run(plan, fam, gpu.from_numpy(np.array(x)).cuda(), F).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))


# ---- a channel count whose transform stages ----------------------------------------------------------------------------------------------
def test_8194_points_need_a_work_buffer():
    """the route restatement of tests/test_fft_route.py (tests/emu_route on libredio_amd/csrc/fft_route.h, and that file's table): no
    in-place run and a work buffer at 8194 points -- what makes a bank plan's fft_stages true"""
    from test_fft_route import TABLE
    assert TABLE[STAGING] == ("global", 0, 1)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_route"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "route_table"), str(STAGING)], capture_output=True, text=True, check=True).stdout
    n, route, in_place_ok, needs_work = out.split()
    assert (int(n), route, int(in_place_ok), int(needs_work)) == (STAGING, "global", 0, 1)


STAGING_SHAPE = (STAGING, 2, 4097)   # H: the oversampled families only


@gpu_test
@pytest.mark.parametrize("order", ["as listed", "growing"])
@pytest.mark.parametrize("fam", FAMILIES)
def test_staging_transform_under_changing_chunks(gpu, redio, fam, order):
    """5 units at 8194 channels on ONE plan at chunk 0 (one pass of every row), min_rows and min_rows + 1, first_row 0 and 3: the scratch
    and the transform's own reservation are sized by the largest pass so far.  "growing" makes the same calls smallest pass first, so
    that the transform's reservation has to grow twice."""
    M, P, H = STAGING_SHAPE
    H = M if fam == "pfb_synth" else H
    min_rows = cut_of(fam, M, P, H)[3]
    chunks = (0, min_rows, min_rows + 1) if order == "as listed" else (min_rows, min_rows + 1, 0)
    x, h, _ = case(fam, M, P, H, 5, 0, True)
    plan = make_plan(redio, fam, h, M, P, H, True)
    assert plan.route == 0
    dx = gpu.from_numpy(np.array(x)).cuda()
    for chunk in chunks:
        plan.set_chunk_rows(chunk)
        for F in (0, 3) if fam != "pfb_synth" else (0,):
            want = case(fam, M, P, H, 5, F, True)[2]
            got = run(plan, fam, dx, F).cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (chunk, F)


@gpu_test
@pytest.mark.parametrize("fam", FAMILIES)
def test_staging_transform_needs_the_reserve_inside_a_capture(gpu, redio, fam):
    """under stream capture at 8194 channels: un-reserved refuses and launches nothing; reserved at a chunk of min_rows + 1 rows it
    captures and replays the bits; with the chunk raised so that a pass exceeds what was reserved it refuses again"""
    M, P, H = STAGING_SHAPE
    H = M if fam == "pfb_synth" else H
    min_rows = cut_of(fam, M, P, H)[3]
    x, h, want = case(fam, M, P, H, 5, 3, True)
    if fam == "pfb_synth":
        want = case(fam, M, P, H, 5, 0, True)[2]
    plan = make_plan(redio, fam, h, M, P, H, True)
    dx = gpu.from_numpy(np.array(x)).cuda()
    out = gpu.full((len(want),), 7.0, dtype=gpu.complex64, device="cuda")
    plan.set_chunk_rows(min_rows + 1)
    assert len(passes_of(cut_of(fam, M, P, H), M, min_rows + 1, 5)) == 3

    def refused():
        with pytest.raises(redio.RedioError) as e:
            with redio.Graph():
                run(plan, fam, dx, 3, out=out)
        assert e.value.code == ERR_NOT_RESERVED
        gpu.cuda.synchronize()

    refused()
    assert bool((out == 7.0).all())  # nothing was launched
    plan.reserve(len(x))
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        run(plan, fam, dx, 3, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    assert redio.lib().redio_malloc_count() == count  # reserved: no enqueue allocated
    plan.set_chunk_rows(0)   # one pass of every row: more than the min_rows + 1 rows reserved
    out.fill_(7.0)
    refused()
    assert bool((out == 7.0).all())
    assert np.array_equal(bits(run(plan, fam, dx, 3, out=out).cpu().numpy()), bits(want))  # un-captured it grows and runs


# ---- small and odd shapes ------------------------------------------------------------------------------------------------------------------
SMALL = [("pfb_synth", M, P, M) for M, P in [(1, 1), (7, 1), (2, 3), (64, 1), (64, 32)]] + \
        [(fam, M, P, H) for fam in ("pfb_os", "pfb_os_synth") for M, P, H in [(1, 1, 1), (7, 1, 7), (7, 3, 1), (12, 2, 7), (64, 4, 1), (64, 4, 63)]]


@gpu_test
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("fam,M,P,H", SMALL)
def test_small_and_odd_shapes(gpu, redio, fam, M, P, H, fused):
    window, hop, unit_out, min_rows = cut_of(fam, M, P, H)
    top = 9
    x, h, _ = case(fam, M, P, H, top, 0, fused, extra=hop - 1)   # a trailing partial row / hop: ignored
    plan = make_plan(redio, fam, h, M, P, H, fused)
    assert plan.route == 0 and not plan.is_fused
    if fam != "pfb_synth":
        assert plan.hop == H
    ins = {off: put(gpu, x, off) for off in (0, 1)}
    obuf = gpu.empty(top * unit_out + 3, dtype=gpu.complex64, device="cuda")
    for units in (0, 1, 9):
        n = (units - 1) * hop + window + hop - 1 if units else window - 1
        answered = plan.nrows(n) * M if fam == "pfb_os" else plan.nout(n)
        assert answered == units * unit_out
        T = units if fam == "pfb_os" else units + min_rows - 1
        for F in (0,) if fam == "pfb_synth" else (0, 1, 2 ** 64 - 1 - T):
            want = want_of(fam, x[:n], h, M, P, H, F, fused)
            assert want.shape == (units * unit_out,)
            for chunk, pairs in ((0, ((0, 0), (1, 0), (0, 1), (1, 1))), (min_rows + 1, ((1, 1),))):
                plan.set_chunk_rows(chunk)
                for off, ooff in pairs:
                    obuf.fill_(7.0)
                    lo = 1 + ooff   # a guard element in front: lo = 1 is 8 bytes past a 16-byte boundary, lo = 2 on one
                    got = run(plan, fam, ins[off][:n], F, out=obuf[lo: lo + len(want)])
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (units, F, chunk, off, ooff)
                    assert (obuf[lo + len(want):] == 7.0).all().item() and (obuf[:lo] == 7.0).all().item(), "wrote outside the output"
