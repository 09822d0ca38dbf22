"""The chain kernel's seam between two sub-tiles (chain_v4.hip, round 12): lane-constant LDS slots computed once per wave, the stream
and the spectra addressed through buffer descriptors on a scalar base, the halo read under the FIR's last chunk and written
branch-free by all 64 lanes, and a prologue that requests everything before its first wait.  Bar: the bits of oracle.chain_fir_fft
(oracle.fir for the stand-alone FIR plan, which runs the same body), with fmaf and with reference rounding, in every case.

The four shapes differ in the halo's lane count (61, 29, 63 and 31 of the wave's 64 lanes move a halo pair, the others move a pair of
new samples onto itself) and in how many park slots share an address register (five at / 5, one at / 1).  Messages of 1 ... 13
blocks are runs of ONE block; the 24 579-block launch is runs of two with a last run of one, so the scalar offsets advance across
a transform inside a run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(127, 5), (63, 5), (127, 1), (63, 1)]  # halo K - D = 122, 58, 126, 62 samples
NBS = (1, 2, 5, 13)
NMAX = max(NBS)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def n_in(k, d, nb):
    return (1024 * nb - 1) * d + k


def ulp_taps(oracle, k):
    """lpf_corrected with one tap one ulp off its mirror: the any-taps twin runs"""
    t = oracle.lpf_corrected(k, 0.08).copy()
    t[k - 1 - 7] = np.nextafter(t[7], np.float32(np.inf), dtype=np.float32)
    assert not np.array_equal(bits(t), bits(t[::-1]))
    return t


_CASES = {}


def case(oracle, k, d, fused, form="palindromic"):
    """taps, an input of NMAX blocks and its oracle spectra, once per case: a message of nb blocks is the prefix, its spectra the first nb rows"""
    key = (k, d, fused, form)
    if key not in _CASES:
        taps = oracle.lpf_corrected(k, 0.08) if form == "palindromic" else ulp_taps(oracle, k)
        x = oracle.synth_iq(0x5EA0 + 7 * k + d, 0, n_in(k, d, NMAX))
        _CASES[key] = (taps, x, oracle.chain_fir_fft(x, taps, d, 1024, fused=fused))
    return _CASES[key]


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_cf32_bits(gpu, redio, oracle, k, d, fused):
    taps, x, want = case(oracle, k, d, fused)
    chain = redio.Chain(taps, d, 1024, fused=fused)
    assert chain.is_fused and chain.kernel_name.startswith(f"chain_v4_kernel<{k},{d},")
    dx = gpu.from_numpy(x).cuda()
    for nb in NBS:
        got = chain(dx[: n_in(k, d, nb)]).cpu().numpy()
        assert got.shape == (nb, 1024)
        assert same_bits(got, want[:nb]), f"({k}, {d}), {nb} blocks"


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_u8_bits(gpu, redio, oracle, k, d, fused):
    taps = oracle.lpf_corrected(k, 0.08)
    raw = np.random.default_rng(0x5EA8 + k + d).integers(0, 256, 2 * n_in(k, d, NMAX), dtype=np.uint8)
    want = oracle.chain_fir_fft(oracle.data_to_samples(raw), taps, d, 1024, fused=fused)
    chain = redio.Chain(taps, d, 1024, fused=fused)
    draw = gpu.from_numpy(raw).cuda()
    for nb in NBS:
        got = chain.from_bytes(draw[: 2 * n_in(k, d, nb)]).cpu().numpy()
        assert same_bits(got, want[:nb]), f"u8 ({k}, {d}), {nb} blocks"


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_anytaps_bits(gpu, redio, oracle, k, d, fused):
    taps, x, want = case(oracle, k, d, fused, "ulp")
    twin = redio.Chain(taps, d, 1024, fused=fused)
    assert twin.is_fused and twin.kernel_name.startswith(f"chain_v4_anytaps_kernel<{k},{d},")
    dx = gpu.from_numpy(x).cuda()
    for nb in NBS:
        assert same_bits(twin(dx[: n_in(k, d, nb)]).cpu().numpy(), want[:nb]), f"any taps ({k}, {d}), {nb} blocks"


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_list_bits(gpu, redio, oracle, k, d, fused):
    """messages of 1, 2 and 5 blocks in one launch, at offsets of their own in the stream: the resident-taps list kernel and its any-taps twin"""
    for form in ("palindromic", "ulp"):
        taps, x, _ = case(oracle, k, d, fused, form)
        chain = redio.Chain(taps, d, 1024, fused=fused)
        dx = gpu.from_numpy(x).cuda()
        offs, nbs = (0, 2 * 1024 * d, 6 * 1024 * d), (1, 2, 5)
        msgs = [dx[o: o + n_in(k, d, nb)] for o, nb in zip(offs, nbs)]
        outs = chain.enqueue_list(msgs)
        for o, nb, got in zip(offs, nbs, outs):
            want = oracle.chain_fir_fft(x[o: o + n_in(k, d, nb)], taps, d, 1024, fused=fused)
            assert same_bits(got.cpu().numpy(), want), f"list, {form} taps ({k}, {d}), message of {nb} blocks"


@pytest.mark.parametrize("k,d", SHAPES)
@pytest.mark.parametrize("fused", [True, False])
def test_offset_view(gpu, redio, oracle, k, d, fused):
    """the first block starts 16 bytes into the allocation: the descriptor's base is the view's, not the allocation's"""
    taps, x, want = case(oracle, k, d, fused)
    chain = redio.Chain(taps, d, 1024, fused=fused)
    base = gpu.zeros(x.size + 2, dtype=gpu.complex64, device="cuda")
    view = base[2:]
    view.copy_(gpu.from_numpy(x))
    assert view.data_ptr() % 16 == 0 and view.data_ptr() == base.data_ptr() + 16
    for nb in (1, 5, 13):
        assert same_bits(chain(view[: n_in(k, d, nb)]).cpu().numpy(), want[:nb]), f"offset view ({k}, {d}), {nb} blocks"


@pytest.mark.parametrize("k,d", [(127, 5), (63, 1)])
@pytest.mark.parametrize("fused", [True, False])
def test_fir_plan(gpu, redio, oracle, k, d, fused):
    """the stand-alone FIR on whole 1024-output blocks runs the chain's body without the transform (three waves per SIMD)"""
    for form in ("palindromic", "ulp"):
        taps, x, _ = case(oracle, k, d, fused, form)
        fir = redio.Fir(taps, d, complex_input=True, fused=fused)
        dx = gpu.from_numpy(x).cuda()
        for nb in (1, 5):
            n = n_in(k, d, nb)
            got = fir(dx[:n]).cpu().numpy()
            want = oracle.fir(x[:n], taps, d, fused=fused)
            assert got.shape == (1024 * nb,)
            assert same_bits(got, want), f"Fir plan, {form} taps ({k}, {d}), {nb} blocks"


NB2 = 24579  # runs of two blocks and a last run of one


@pytest.fixture(scope="module")
def long_stream(gpu, redio):
    x = redio.synth_iq(0x5EA2B10C, 0, n_in(127, 5, NB2))
    yield x
    del x
    gpu.cuda.empty_cache()


@pytest.mark.parametrize("fused", [True, False])
def test_runs_of_two(gpu, redio, oracle, long_stream, fused):
    """one launch whose waves run two blocks each: the stream's and the spectra's scalar offsets advance across a transform"""
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=fused)
    assert chain.blocks_per_wave(NB2) == 2 and chain.launch_waves(NB2) == (NB2 + 1) // 2
    got = chain(long_stream)
    assert got.shape == (NB2, 1024)
    mid = (NB2 // 4) * 2
    for r0, r1 in ((0, 2), (mid, mid + 2), (NB2 - 3, NB2 - 1), (NB2 - 1, NB2)):  # first, a middle, the last full and the shorter last run
        lo = r0 * 1024 * 5
        xs = long_stream[lo: lo + n_in(127, 5, r1 - r0)].cpu().numpy()
        want = oracle.chain_fir_fft(xs, taps, 5, 1024, fused=fused)
        assert same_bits(got[r0:r1].cpu().numpy(), want), f"blocks {r0} ... {r1 - 1} differ from the oracle"
