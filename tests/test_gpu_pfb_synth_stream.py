"""The synthesis filterbank as a stream (redio_pfb_synth_stream_*): any segmentation of the channel values concatenates to the one-shot
result of the oracle restatement (tests/pfb_synth_ref.py), bit for bit, on the wave kernel and on the two-pass route."""
import numpy as np
import pytest

import pfb_synth_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED5178


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def feed(gpu, st, xd, cuts, M, P):
    """feed xd in pieces of the given lengths; checks nout and pending against the ref's arithmetic after every piece"""
    outs, pos = [], 0
    for n in cuts:
        before = ref.nout(pos, M, P)
        pos += n
        after = ref.nout(pos, M, P)
        assert st.nout(n) == after - before
        y = st(xd[pos - n: pos])
        assert y.numel() == after - before
        outs.append(y.cpu().numpy())
        # carried: everything from the first row not yet produced
        assert st.pending == pos - after
    return np.concatenate(outs) if outs else np.empty(0, np.complex64)


def segmentations(rng, n, M, P):
    k = 3 * M + 5
    yield "ones", [1] * k + [n - k]
    for name, m in (("M-1", M - 1), ("M", M), ("PM-1", P * M - 1)):
        cuts = [m] * (n // m)
        if n % m:
            cuts.append(n % m)
        yield name, cuts
    for j in range(3):
        cuts, left = [], n
        while left:
            c = int(min(left, rng.integers(1, 3 * P * M)))
            cuts.append(c)
            left -= c
        yield f"random{j}", cuts


@pytest.mark.parametrize("M,P,fused,unfused", [(64, 4, True, False), (64, 4, True, True), (64, 16, False, False), (64, 16, False, True),
                                               (32, 8, True, False), (12, 3, False, False)])
def test_any_segmentation_concatenates_to_the_one_shot_result(gpu, redio, oracle, M, P, fused, unfused):
    rng = np.random.default_rng(SEED + M + P)
    n = (2 * P + 37) * M + M // 2  # ends inside a row
    xh = oracle.synth_iq(SEED, M, n)
    h = oracle.synth_f32(3, P, M * P)
    want = ref.synth(xh, h, M, P, fused)
    xd = gpu.from_numpy(xh).cuda()
    plan = redio.Synthesizer(h, M, P, fused=fused)
    if unfused:
        plan.set_unfused(True)
    assert plan.route == (0 if unfused else ref.route(M, P))
    st = redio.SynthesizerStream(plan)
    assert st.pending == 0
    for name, cuts in segmentations(rng, n, M, P):
        assert sum(cuts) == n
        got = feed(gpu, st, xd, cuts, M, P)
        assert np.array_equal(bits(got), bits(want)), name
        assert st.pending == n - len(want)
        st.reset()
        assert st.pending == 0 and st.nout(P * M - 1) == 0 and st.nout(P * M) == M
    # after a reset in mid-stream the history is gone
    st(xd[: P * M - 1])
    st.reset()
    got = feed(gpu, st, xd, [n], M, P)
    assert np.array_equal(bits(got), bits(want))
