"""The oversampled channelizer as a stream (redio_pfb_os_stream_*): any segmentation of the samples concatenates to the one-call rows
of the oracle restatement (tests/pfb_os_ref.py) with first_row = 0, bit for bit, on the wave kernel and on the two-pass route; the
shift goes on across messages that end on odd row counts; reset; pending and nout against the ref's stream model."""
import numpy as np
import pytest

import pfb_os_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0534


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feed(st, xd, cuts, M, P, H):
    """feed xd in pieces of the given lengths; checks nout and pending against the ref's arithmetic after every piece"""
    outs, pos = [], 0
    for n in cuts:
        before = ref.nrows(pos, M, P, H)
        pos += n
        after = ref.nrows(pos, M, P, H)
        assert st.nout(n) == (after - before) * M
        y = st(xd[pos - n: pos])
        assert y.numel() == (after - before) * M
        outs.append(y.cpu().numpy())
        assert st.pending == pos - after * H  # carried: everything from the next row's first sample on
    return np.concatenate(outs) if outs else np.empty(0, np.complex64)


def whole(n, m):
    return [m] * (n // m) + ([n % m] if n % m else [])


def segmentations(rng, n, M, P, H):
    yield "ones", [1] * (M * P + 2 * H + 3) + [n - (M * P + 2 * H + 3)]
    for m in (31, 32, 33, M * P - 1, M * P):
        yield str(m), whole(n, m)
    yield "empty messages", [0, M * P - 1, 0, 1, 0, H, 0, n - M * P - H]
    yield "odd row counts", [M * P, H, 2 * H, 3 * H, H - 1, 1, n - M * P - 7 * H]  # 1, 1, 2, 3, 0, 1 rows: the row index is odd at most seams
    for j in range(2):
        cuts, left = [], n
        while left:
            c = int(min(left, rng.integers(1, 2 * P * M)))
            cuts.append(c)
            left -= c
        yield f"random{j}", cuts


@pytest.mark.parametrize("M,P,H,fused,unfused", [(64, 4, 32, True, False), (64, 4, 32, True, True), (64, 16, 32, False, False),
                                                  (64, 8, 48, True, False), (32, 8, 16, False, False), (12, 3, 5, True, False)])
def test_any_segmentation_concatenates_to_the_one_call_rows(gpu, redio, oracle, M, P, H, fused, unfused):
    rng = np.random.default_rng(SEED + M + P + H)
    n = M * P + 45 * H + H // 2  # 46 rows; ends inside a hop
    xh = oracle.synth_iq(SEED, M, n)
    h = oracle.synth_f32(3, P, M * P)
    want = ref.channelize(xh, h, M, P, H, 0, fused).reshape(-1)
    xd = gpu.from_numpy(xh).cuda()
    plan = redio.OversampledChannelizer(h, M, P, H, fused=fused)
    if unfused:
        plan.set_unfused(True)
    assert plan.route == (0 if unfused else ref.route(M, P, H))
    st = redio.OversampledChannelizerStream(plan)
    assert st.pending == 0
    for name, cuts in segmentations(rng, n, M, P, H):
        assert sum(cuts) == n
        got = feed(st, xd, cuts, M, P, H)
        assert np.array_equal(bits(got), bits(want)), name
        assert st.pending == n - 46 * H
        st.reset()
        assert st.pending == 0 and st.nout(P * M - 1) == 0 and st.nout(P * M) == M
    # after a reset in mid-stream both the samples and the row index are gone: three rows in, then the stream from its start
    st(xd[: M * P + 2 * H])
    st.reset()
    got = feed(st, xd, [n], M, P, H)
    assert np.array_equal(bits(got), bits(want))


def test_the_stream_matches_the_refs_stream_model(gpu, redio, oracle):
    M, P, H = 64, 4, 32
    xh = oracle.synth_iq(SEED, 3, 2000)
    h = oracle.synth_f32(3, 7, M * P)
    xd = gpu.from_numpy(xh).cuda()
    st = redio.OversampledChannelizerStream(redio.OversampledChannelizer(h, M, P, H))
    model = ref.StreamModel(h, M, P, H, True)
    pos = 0
    for c in (100, 155, 1, 32, 0, 353, 31, 700, 628):
        assert st.nout(c) == model.nout(c)
        got = st(xd[pos: pos + c]).cpu().numpy()
        assert np.array_equal(bits(got), bits(model.feed(xh[pos: pos + c]))) and st.pending == model.pending
        pos += c
    assert pos == 2000 and model.row == ref.nrows(2000, M, P, H)
