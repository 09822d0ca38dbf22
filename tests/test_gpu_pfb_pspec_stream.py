"""redio_pfb_pspec_stream_*: the polyphase spectrometer fed as a stream in pieces gives the bits of one call on the whole, from cf32
samples and from u8 I/Q bytes, on a fused and a generic shape, and again after reset()."""
import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F5D


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("M,P,K", [(64, 16, 17), (64, 4, 3), (128, 8, 5)])
def test_stream_gives_the_one_shot_bits(gpu, redio, oracle, M, P, K, u8):
    """messages of 1 sample, an odd count, less than a row, a window less a few, whole hops and several windows"""
    W, H = ref.shape(M, P, K)
    lens = [1, 7, M - 3, W - 9, 1, H, W, W + 1, 3 * H + 5, 333, 2 * W + H - 1, 1, H - 1]
    h = oracle.synth_f32(9, 0, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    if u8:
        raw = np.random.default_rng(SEED).integers(0, 256, 2 * sum(lens), dtype=np.uint8)
        d = gpu.from_numpy(raw).cuda()
        whole, want = plan.from_bytes(d), ref.spectrum_u8(raw, h, M, P, K, True)
    else:
        x = oracle.synth_iq(SEED, 0, sum(lens))
        d = gpu.from_numpy(x).cuda()
        whole, want = plan(d), ref.spectrum(x, h, M, P, K, True)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(want))
    s = redio.Stream(plan, u8=u8)
    e = 2 if u8 else 1
    for attempt in range(2):  # reset() starts over: the second pass repeats the first
        pos, outs, made = 0, [], 0
        for n in lens:
            expect = ref.nrows(pos + n, M, P, K) - made
            assert s.nout(n) == expect * M
            y = s(d[e * pos: e * (pos + n)])
            assert y.dtype == gpu.float32 and y.numel() == expect * M
            outs.append(y.clone())
            pos += n
            made += expect
            assert s.pending == pos - made * H
        assert gpu.equal(gpu.cat(outs), whole.reshape(-1)), attempt
        s.reset()
        assert s.pending == 0
