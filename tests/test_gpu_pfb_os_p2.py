"""redio_pfb_os_* with REDIO_PFB_OS_BLOCK on the GPU: the workgroup kernel (route 2) of the one-kernel channelizer shapes at hop
nchan / 2, bit for bit against the oracle restatement (tests/pfb_os_ref.channelize; shared inputs: tests/pfb_os_p2_ref.py) -- every
shape over the row counts around an iteration, a stream and a workgroup with four first rows, both folds, buffers 8 bytes off 16-byte
alignment, the same shapes without the flag, flagged shapes that have no workgroup form, and set_unfused there and back."""
import numpy as np
import pytest

import pfb_os_p2_ref as p2
import pfb_os_ref as ref

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def put(gpu, a, off):
    """the values on the device at a 16-byte aligned address (off = 0) or one 8 bytes past it (off = 1)"""
    buf = gpu.zeros(len(a) + 2, dtype=gpu.complex64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off: off + len(a)]
    v.copy_(gpu.from_numpy(np.array(a)))
    return v


def firsts(rows):
    return (0, 1, 7, 2 ** 64 - 1 - rows)


def run_lengths(gpu, plan, M, P, fused, offsets, want_route):
    """every row count of rows_list(M) with every first row; offsets: (input, output) placements, 1 = 8 bytes off 16-byte alignment"""
    H = M // 2
    x, _, _ = p2.case(M, P, fused)
    top = max(p2.rows_list(M))
    ins = {off: put(gpu, x, off) for off in {o for o, _ in offsets}}
    obuf = gpu.empty(top * M + 2, dtype=gpu.complex64, device="cuda")
    assert plan.route == want_route and not plan.is_fused and plan.hop == H
    for rows in p2.rows_list(M):
        n = p2.n_in(M, P, rows)
        extra = H - 1 if rows else 0  # samples short of one more row are not read
        assert plan.nrows(n) == plan.nrows(n + extra) == ref.nrows(n, M, P, H) == rows
        for F in firsts(rows):
            want = p2.want_rows(M, P, fused, F & 1)[:rows]
            for off, ooff in offsets:
                obuf.fill_(7.0)
                got = plan(ins[off][: n + extra], first_row=F, out=obuf[ooff:])
                assert got.shape == (rows, M)
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (rows, F, off, ooff)
                assert (obuf[ooff + rows * M:] == 7.0).all().item() and (obuf[:ooff] == 7.0).all().item(), "wrote outside the output"
                assert plan.route == want_route


@pytest.mark.parametrize("M,P", p2.SHAPES)
def test_every_shape_against_the_ref(gpu, redio, M, P):
    _, h, _ = p2.case(M, P, True)
    plan = redio.OversampledChannelizer(h, M, P, M // 2, fused=True, one_kernel=True)
    assert p2.route(M, P, M // 2, True) == 2 == redio.OversampledChannelizer.BLOCK
    run_lengths(gpu, plan, M, P, True, [(0, 0)], 2)


def test_the_shared_reference_is_the_contract(gpu, redio):
    """the cases above share branch sums and take the shift from the parity of F: pfb_os_ref.channelize on a call's own input gives
    the same rows"""
    M, P = 128, 4
    x, h, _ = p2.case(M, P, True)
    for rows, F in ((17, 7), (65, 2 ** 64 - 66)):
        want = ref.channelize(x[: p2.n_in(M, P, rows)], h, M, P, M // 2, F, True)
        assert np.array_equal(bits(want), bits(p2.want_rows(M, P, True, F & 1)[:rows]))


@pytest.mark.parametrize("M,P", [(32, 8), (128, 16), (256, 4), (512, 16), (1024, 8)])
def test_the_unfused_fold(gpu, redio, M, P):
    """multiply and add rounded separately (no REDIO_FIR_FUSED): one shape per channel count"""
    _, h, _ = p2.case(M, P, False)
    plan = redio.OversampledChannelizer(h, M, P, M // 2, fused=False, one_kernel=True)
    run_lengths(gpu, plan, M, P, False, [(0, 0)], 2)


@pytest.mark.parametrize("M,P", [(32, 4), (128, 8), (256, 16), (512, 4), (1024, 4)])
def test_buffers_eight_bytes_off_sixteen_byte_alignment(gpu, redio, M, P):
    """the kernel takes its 8-byte loads (512 and 1024 channels: the other load form) and 8-byte stores; the same bits, still route 2"""
    _, h, _ = p2.case(M, P, True)
    plan = redio.OversampledChannelizer(h, M, P, M // 2, fused=True, one_kernel=True)
    run_lengths(gpu, plan, M, P, True, [(1, 0), (0, 1), (1, 1)], 2)


@pytest.mark.parametrize("M,P", p2.SHAPES)
def test_without_the_flag_the_route_is_0_and_the_bits_are_equal(gpu, redio, M, P):
    x, h, _ = p2.case(M, P, True)
    rows = max(p2.rows_list(M))
    xd = put(gpu, x, 0)
    plain = redio.OversampledChannelizer(h, M, P, M // 2, fused=True)
    block = redio.OversampledChannelizer(h, M, P, M // 2, fused=True, one_kernel=True)
    assert plain.route == 0 == p2.route(M, P, M // 2, False) and not plain.is_fused and block.route == 2
    for F in (0, 1):
        a, b = plain(xd, first_row=F).cpu().numpy(), block(xd, first_row=F).cpu().numpy()
        assert a.shape == b.shape == (rows, M)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(p2.want_rows(M, P, True, F)))


@pytest.mark.parametrize("M,P,H,want", [(256, 8, 64, 0), (100, 3, 50, 0), (64, 8, 32, 1), (128, 5, 64, 0), (2048, 4, 1024, 0)] +
                         [(M, P, M // 2, 0) for M, P in p2.LEFT_OUT])
def test_the_flag_changes_nothing_on_other_shapes(gpu, redio, oracle, M, P, H, want):
    assert p2.route(M, P, H, True) == want
    rows = 37
    x = oracle.synth_iq(p2.SEED, M + P, M * P + H * (rows - 1) + 1)
    h = oracle.synth_f32(3, M + P, M * P)
    xd = gpu.from_numpy(x).cuda()
    plain = redio.OversampledChannelizer(h, M, P, H, fused=True)
    block = redio.OversampledChannelizer(h, M, P, H, fused=True, one_kernel=True)
    assert plain.route == block.route == want and block.is_fused == plain.is_fused == (want == 1)
    a, b = plain(xd, first_row=3).cpu().numpy(), block(xd, first_row=3).cpu().numpy()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(ref.channelize(x, h, M, P, H, 3, True)))


def test_set_unfused_there_and_back(gpu, redio):
    M, P = 256, 8
    x, h, _ = p2.case(M, P, True)
    xd = put(gpu, x, 0)
    plan = redio.OversampledChannelizer(h, M, P, M // 2, fused=True, one_kernel=True)
    want = p2.want_rows(M, P, True, 1)
    count = redio.lib().redio_malloc_count()
    plan.reserve(xd.numel())  # route 2: nothing to reserve
    one = plan(xd, first_row=1).cpu().numpy()
    assert plan.route == 2 and redio.lib().redio_malloc_count() == count
    plan.set_unfused(True)
    assert plan.route == 0 and not plan.is_fused
    two = plan(xd, first_row=1).cpu().numpy()
    assert redio.lib().redio_malloc_count() > count  # route 0 took its scratch
    plan.set_unfused(False)
    assert plan.route == 2 and not plan.is_fused
    back = plan(xd, first_row=1).cpu().numpy()
    for got in (one, two, back):
        assert np.array_equal(bits(got), bits(want))
