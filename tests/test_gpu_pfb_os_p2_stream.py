"""The oversampled channelizer as a stream (redio_pfb_os_stream_*) over a route-2 plan (REDIO_PFB_OS_BLOCK): pieces of length 0, short
of a window, odd lengths and several windows concatenate to the one-shot call with first_row = 0, bit for bit; the row index is
carried, so the parity of the shift flips across messages that hold an odd number of rows."""
import numpy as np
import pytest

import pfb_os_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0B54


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feed(st, xd, cuts, M, P, H):
    outs, pos, odd = [], 0, 0
    for n in cuts:
        before = ref.nrows(pos, M, P, H)
        pos += n
        after = ref.nrows(pos, M, P, H)
        assert st.nout(n) == (after - before) * M
        y = st(xd[pos - n: pos])
        assert y.numel() == (after - before) * M
        outs.append(y.cpu().numpy())
        assert st.pending == pos - after * H
        odd += before & 1 and after > before  # a message whose first row is an odd row of the stream
    return (np.concatenate(outs) if outs else np.empty(0, np.complex64)), odd


@pytest.mark.parametrize("M,P", [(128, 8), (1024, 4)])
def test_pieces_concatenate_to_the_one_shot_call(gpu, redio, oracle, M, P):
    H = M // 2
    rows = 75
    n = M * P + (rows - 1) * H + H // 2  # ends inside a hop
    xh = oracle.synth_iq(SEED, M, n)
    h = oracle.synth_f32(3, P, M * P)
    want = ref.channelize(xh, h, M, P, H, 0, True).reshape(-1)
    xd = gpu.from_numpy(xh).cuda()
    plan = redio.OversampledChannelizer(h, M, P, H, one_kernel=True)
    assert plan.route == 2
    one = plan(xd, first_row=0).cpu().numpy().reshape(-1)
    assert np.array_equal(bits(one), bits(want))
    st = redio.OversampledChannelizerStream(plan)
    W = M * P
    segs = {
        "short of a window": [0, W - 1, 0, 1, 0, H, n - W - H],
        "odd row counts": [W, H, 2 * H, 3 * H, H - 1, 1, 5 * H + 3, n - W - 12 * H - 3],
        "odd lengths": [333] * (n // 333) + ([n % 333] if n % 333 else []),
        "several windows": [3 * W + 1, 2 * W + 7, n - 5 * W - 8],
        "whole": [n],
    }
    flips = 0
    for name, cuts in segs.items():
        assert sum(cuts) == n and all(c >= 0 for c in cuts), name
        got, odd = feed(st, xd, cuts, M, P, H)
        flips += odd
        assert np.array_equal(bits(got), bits(want)), name
        assert st.pending == n - rows * H and plan.route == 2
        st.reset()
        assert st.pending == 0
    assert flips >= 3  # messages began on odd rows of the stream: the shift's parity came from the carried row index
