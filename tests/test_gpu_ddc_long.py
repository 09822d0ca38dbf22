"""The tuner (redio_ddc_*) on the device at long filters, bit for bit against the oracle's mul_vecs + fir (tests/ddc_ref.py): the last
tap count the chunked route takes at each decimation (a tile of 150 KiB, table indices up to 18279 entries past the workgroup's base)
and the direct route one tap later, the chunk walk around its chunk size, and windows of thousands of samples with infinities on
either side of them.  The oracle's cost is outputs x taps, so every case asks for one whole tile and a partial one and never
shortens the filter."""
import numpy as np
import pytest

import ddc_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EEDDDC4
DECIMS = sorted(ref.CHUNKED_R)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_special(got, want):
    """bit for bit, NaNs by position (as test_gpu_ddc.py)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


def firsts(L):
    """first_index values by the table base (first mod L) of the first workgroup: L - 1 (odd for an even period: 8-byte table loads,
    and the farthest the indices reach), an odd one and an even one behind 2^32"""
    return [0, 2 ** 32] if L == 1 else [L - 1, 2 ** 32 * L + 1, 2 ** 40 * L + 6 % L]


class Inputs:
    """n samples as cf32 and as u8 bytes, each once at an aligned address and once off it (cf32: one sample; u8: one sample and one
    byte), and an output buffer"""

    def __init__(self, gpu, oracle, rng, n, n_out):
        self.gpu = gpu
        self.raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
        self.host = {False: oracle.synth_iq(SEED, n % 1000, n), True: oracle.data_to_samples(self.raw)}
        self.views = {}
        for u8, src, offs in ((False, self.host[False], (0, 1)), (True, self.raw, (0, 2, 1))):
            buf = gpu.zeros(len(src) + 4, dtype=gpu.uint8 if u8 else gpu.complex64, device="cuda")
            for off in offs:
                b = buf.clone()
                b[off: off + len(src)] = gpu.from_numpy(src).cuda()
                self.views[(u8, off)] = b[off: off + len(src)]
        self.obuf = gpu.empty(n_out + 2, dtype=gpu.complex64, device="cuda")

    def check(self, plan, u8, first, want, tag):
        run = plan.from_bytes if u8 else plan
        for (v8, off), x in self.views.items():
            if v8 == u8:
                ooff = 1 if off else 0
                got = run(x, first=first, out=self.obuf[ooff:])
                assert got.numel() == len(want)
                assert np.array_equal(bits(got.cpu().numpy()), bits(want)), tag + (off,)


@pytest.mark.parametrize("D,K,route", [(D, ref.last_chunked(D) + more, 2 + more) for D in DECIMS for more in (0, 1)])
def test_the_lds_limit_and_the_direct_route_behind_it(gpu, redio, oracle, D, K, route):
    """the pinned table of tests/test_ddc_cpu.py on the device: periods 1, 3 and 65536, every base of firsts(), cf32 and bytes"""
    assert {1: 15008, 2: 15008, 3: 14640, 4: 13968, 5: 13152, 8: 13968, 10: 13168}[D] == K - (route - 2)
    TO = ref.tile_out(K, D)
    assert ref.route(K, D) == route and TO == (256 * ref.CHUNKED_R[D] if route == 2 else 256)
    if route == 2:
        assert ref.lds_elems(K, D) * 8 <= ref.CHUNKED_LDS_MAX < ref.lds_elems(K + 1, D) * 8 and ref.tile_in(K, D) + 2 <= ref.TABLE_EXT
    n_out = TO + 1 + 4
    n = (n_out - 1) * D + K
    taps = oracle.synth_f32(3, K, K)
    inp = Inputs(gpu, oracle, np.random.default_rng(SEED + 977 * K + D), n, n_out)
    parity = set()
    for L in (1, 3, 65536):
        w = oracle.synth_iq(7, L, L)
        plans = {fused: redio.Ddc(w, taps, D, fused=fused) for fused in (False, True)}
        for fi, first in enumerate(firsts(L)):
            parity.add((L, first % L & 1))
            for u8 in (False, True):
                fused = bool((fi + u8) & 1)  # the folds alternate: every (period, sample type) meets both
                plan = plans[fused]
                assert plan.route == route and plan.period == L
                want = ref.ddc(inp.host[u8], w, taps, D, fused, first)
                assert len(want) == n_out == plan.nout(n)
                inp.check(plan, u8, first, want, (L, first, u8, fused))
    assert parity == {(1, 0), (3, 0), (3, 1), (65536, 0), (65536, 1)}


@pytest.mark.parametrize("D", DECIMS)
def test_the_chunk_walk_behind_the_mixing_loader(gpu, redio, oracle, D):
    """tap counts one under, at and one over the whole-chunk size, one under six chunks, and 4097 (256 chunks of 16 and one tap)"""
    chw = ref.chw(D)
    assert chw == {1: 16, 2: 16, 3: 24, 4: 16, 5: 40, 8: 16, 10: 40}[D]
    L, first = 4099, 2 ** 32 + 5
    w = oracle.synth_iq(7, L, L)
    TO = ref.tile_out(chw, D)
    n_out = TO + 1 + 4
    for case, K in enumerate([chw - 1, chw, chw + 1, 6 * chw - 1, 4097]):
        assert ref.route(K, D) == 2 and ref.tile_out(K, D) == TO
        n = (n_out - 1) * D + K
        taps = oracle.synth_f32(3, K, K)
        inp = Inputs(gpu, oracle, np.random.default_rng(SEED + 977 * K + D), n, n_out)
        for u8 in (False, True):
            fused = bool((case + u8) & 1)
            plan = redio.Ddc(w, taps, D, fused=fused)
            assert plan.route == 2
            inp.check(plan, u8, first, ref.ddc(inp.host[u8], w, taps, D, fused, first), (K, u8, fused))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("K,D", [(15007, 1), (13151, 5)])
def test_no_tap_beyond_the_filter_is_multiplied_at_length(gpu, redio, oracle, K, D, fused):
    """one tap under the limit, so the taps' zero padding holds one tap: an infinity in the sample just before the window of output i
    and one in the sample just behind it (the one the padded tap would meet) leave output i the finite value it has without them; a
    NaN in the last tap reaches every output"""
    assert ref.route(K, D) == 2 and K % 16 == 15
    TO = ref.tile_out(K, D)
    L, first = 65536, 65535
    n_out = TO + 1 + 4
    n = (n_out - 1) * D + K
    taps, w, clean = oracle.synth_f32(3, K, K), oracle.synth_iq(7, L, L), oracle.synth_iq(SEED, 9, n)
    want_clean = ref.ddc(clean, w, taps, D, fused, first)
    assert np.isfinite(want_clean.view(np.float32)).all() and len(want_clean) == n_out
    plan = redio.Ddc(w, taps, D, fused=fused)
    for i in (1, TO // 2 + 3, TO - 1, TO + 2):  # first and last lanes of the whole tile, the partial tile
        lo, hi = i * D, i * D + K - 1
        xh = clean.copy()
        xh[lo - 1] = xh[hi + 1] = np.inf
        want = ref.ddc(xh, w, taps, D, fused, first)
        got = plan(gpu.from_numpy(xh).cuda(), first=first).cpu().numpy()
        assert same_special(got, want)
        assert bits(got[i: i + 1]).tolist() == bits(want_clean[i: i + 1]).tolist() and not np.isfinite(want.view(np.float32)).all()
    bad = taps.copy()
    bad[K - 1] = np.nan
    got = redio.Ddc(w, bad, D, fused=fused)(gpu.from_numpy(clean).cuda(), first=first).cpu().numpy()
    assert same_special(got, ref.ddc(clean, w, bad, D, fused, first))
    assert np.isnan(got.view(np.float32)).all()
