"""The oversampled channelizer's workgroup kernel (route 2) on and above its launch geometry's floor of 64 rows per stream: 32 x 4
(eight streams per workgroup) and 256 x 4 (one) at a row count just past 64 * 4 * CUs * G, where the runs grow to 80 rows (five
iterations: the pair loop's single-iteration end) and the last stream is short, and at one in the middle of the floor's range.  Every
row compared on the device with the same plan sent down route 0 (which the existing tests hold to the oracle); the first and the last
64 rows also against the oracle restatement."""
import numpy as np
import pytest

import pfb_os_p2_ref as p2
import pfb_os_ref as ref

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("where", ["past the floor", "middle"])
@pytest.mark.parametrize("M,P", [(32, 4), (256, 4)])
def test_launch_on_and_above_the_floor(gpu, redio, M, P, where):
    H, F = M // 2, 1
    G, TR = p2.shape_consts(M)
    cus = gpu.cuda.get_device_properties(0).multi_processor_count
    full = 64 * 4 * cus * G
    rows = full + 17 if where == "past the floor" else full // 2 + 9
    rps = p2.rows_per_stream(rows, cus, M)
    assert rps == (80 if where == "past the floor" else 64) and rows % rps  # the last stream is short
    n = p2.n_in(M, P, rows)
    h = p2.case(M, P, True)[1]
    x = redio.synth_iq(p2.SEED, M, n)
    plan = redio.OversampledChannelizer(h, M, P, H, fused=True, one_kernel=True)
    assert plan.route == 2 and plan.nrows(n) == rows
    out = gpu.full((rows * M + 2,), 7.0, dtype=gpu.complex64, device="cuda")
    got = plan(x, first_row=F, out=out)
    assert got.shape == (rows, M) and (out[rows * M:] == 7.0).all().item()
    plan.set_unfused(True)
    assert plan.route == 0
    two = plan(x, first_row=F)
    assert gpu.equal(gpu.view_as_real(got).view(gpu.int32), gpu.view_as_real(two).view(gpu.int32))
    xh = x.cpu().numpy()
    first = ref.channelize(xh[: p2.n_in(M, P, 64)], h, M, P, H, F, True)
    last = ref.channelize(xh[(rows - 64) * H:], h, M, P, H, F + rows - 64, True)
    assert first.shape == last.shape == (64, M)
    assert np.array_equal(bits(got[:64].cpu().numpy()), bits(first))
    assert np.array_equal(bits(got[rows - 64:].cpu().numpy()), bits(last))
