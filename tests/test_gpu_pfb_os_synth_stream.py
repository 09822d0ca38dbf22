"""The oversampled synthesis bank as a stream (redio_pfb_os_synth_stream_*): any segmentation of the channel values concatenates to the
one-call output of the oracle restatement (tests/pfb_os_synth_ref.py) with first_row = 0, bit for bit, on the wave kernel and on the
two-pass route; the row index goes on across messages that end on odd row counts and inside a row; reset; pending and nout against the
ref's stream model."""
import numpy as np
import pytest

import pfb_os_synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0535


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feed(st, xd, cuts, M, P, H):
    """feed xd in pieces of the given lengths; checks nout and pending against the ref's arithmetic after every piece"""
    outs, pos = [], 0
    for n in cuts:
        before = ref.nhops(pos, M, P, H)
        pos += n
        after = ref.nhops(pos, M, P, H)
        assert st.nout(n) == (after - before) * H
        y = st(xd[pos - n: pos])
        assert y.numel() == (after - before) * H
        outs.append(y.cpu().numpy())
        assert st.pending == pos - after * M  # carried: L - 1 whole rows and the values of a partial one
    return np.concatenate(outs) if outs else np.empty(0, np.complex64)


def whole(n, m):
    return [m] * (n // m) + ([n % m] if n % m else [])


def segmentations(rng, n, M, P, H):
    W = ref.nrows_per_hop(M, P, H) * M
    yield "ones", [1] * (W + 2 * M + 3) + [n - (W + 2 * M + 3)]
    for m in (M - 1, M, 7 * M, W - 1, W):
        yield str(m), whole(n, m)
    yield "empty messages", [0, W - 1, 0, 1, 0, M, 0, n - W - M]
    yield "odd row counts", [W, M, 2 * M, 3 * M, M - 1, 1, n - W - 7 * M]  # 1, 1, 2, 3, 0, 1 hops: the row index is odd at most seams
    for j in range(2):
        cuts, left = [], n
        while left:
            c = int(min(left, rng.integers(1, 2 * W)))
            cuts.append(c)
            left -= c
        yield f"random{j}", cuts


@pytest.mark.parametrize("M,P,H,fused,unfused", [(64, 4, 32, True, False), (64, 4, 32, True, True), (64, 16, 32, False, False),
                                                  (64, 4, 48, True, False), (32, 3, 20, False, False), (12, 2, 5, True, False)])
def test_any_segmentation_concatenates_to_the_one_call_output(gpu, redio, oracle, M, P, H, fused, unfused):
    rng = np.random.default_rng(SEED + M + P + H)
    L = ref.nrows_per_hop(M, P, H)
    n = (L + 45) * M + M // 2  # 46 hops; ends inside a row
    Xh = oracle.synth_iq(SEED, M, n)
    h = oracle.synth_f32(3, P, M * P)
    want = ref.synth(Xh, h, M, P, H, 0, fused)
    Xd = gpu.from_numpy(Xh).cuda()
    plan = redio.OversampledSynthesizer(h, M, P, H, fused=fused)
    if unfused:
        plan.set_unfused(True)
    assert plan.route == (0 if unfused else ref.route(M, P, H))
    st = redio.OversampledSynthesizerStream(plan)
    assert st.pending == 0
    for name, cuts in segmentations(rng, n, M, P, H):
        assert sum(cuts) == n
        got = feed(st, Xd, cuts, M, P, H)
        assert np.array_equal(bits(got), bits(want)), name
        assert st.pending == n - 46 * M
        st.reset()
        assert st.pending == 0 and st.nout(L * M - 1) == 0 and st.nout(L * M) == H
    # after a reset in mid-stream both the rows and the row index are gone: three hops in, then the stream from its start
    st(Xd[: (L + 2) * M])
    st.reset()
    got = feed(st, Xd, [n], M, P, H)
    assert np.array_equal(bits(got), bits(want))


def test_the_stream_matches_the_refs_stream_model(gpu, redio, oracle):
    M, P, H = 64, 4, 32
    Xh = oracle.synth_iq(SEED, 3, 4000)
    h = oracle.synth_f32(3, 7, M * P)
    Xd = gpu.from_numpy(Xh).cuda()
    st = redio.OversampledSynthesizerStream(redio.OversampledSynthesizer(h, M, P, H))
    model = ref.StreamModel(h, M, P, H, True)
    pos = 0
    for c in (1, 63, 64, 500, 0, 353, 31, 1700, 1288):
        assert st.nout(c) == model.nout(c)
        got = st(Xd[pos: pos + c]).cpu().numpy()
        assert np.array_equal(bits(got), bits(model.feed(Xh[pos: pos + c]))) and st.pending == model.pending
        pos += c
    assert pos == 4000 and model.row == ref.nhops(4000, M, P, H)
