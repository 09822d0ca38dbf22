"""The two forms of the chain-form kernels (chain_v4.hip): bit-palindromic taps stay resident in scalar registers
(chain_v4_kernel, chain_v4_list_kernel), any other taps run the any-taps twins (chain_v4_anytaps_kernel, chain_v4_anytaps_list_kernel).
The plan decides once, at creation, by comparing the 32-bit patterns of taps[i] and taps[K-1-i]; every launch path honours it.
Bar: the bits of oracle.chain_fir_fft / oracle.fir with the same taps, for both forms, every shape and both roundings; where the
taps hold a NaN, NaNs in the same places and the bits of everything else.  The palindromic taps are random with all values
distinct, so a tap map that is off by one changes bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(127, 5), (63, 5), (127, 3), (127, 1), (63, 1)]
NBLOCKS = (1, 4, 5)  # one short run, one full run, a full run plus a one-block run
FORMS = ("palindromic", "ulp", "signed_zero", "quirk_nan")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(g, w):
    """identical bits wherever the oracle's value is no NaN, a NaN exactly where it has one (payloads are not compared)"""
    g, w = np.ascontiguousarray(g).view(np.float32), np.ascontiguousarray(w).view(np.float32)
    wn = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), wn) and np.array_equal(bits(g)[~wn], bits(w)[~wn])


def bit_palindromic(t):
    return np.array_equal(bits(t), bits(t[::-1]))


def make_taps(oracle, k, form):
    if form == "quirk_nan":
        t = oracle.lpf(k, 0.08)
        assert np.isnan(t[1]) and not np.isnan(t[k - 2])
        return t
    rng = np.random.default_rng(0x7A95 + k)
    half = rng.uniform(-0.5, 0.5, (k + 1) // 2).astype(np.float32)
    assert len(np.unique(bits(half))) == len(half) and not np.any(half == 0)
    t = np.empty(k, np.float32)
    t[: len(half)] = half
    t[k - len(half):] = half[::-1]  # a copy of the bits
    assert bit_palindromic(t)
    if form == "ulp":
        t[k - 1 - 7] = np.nextafter(t[7], np.float32(np.inf), dtype=np.float32)
    elif form == "signed_zero":
        t[3], t[k - 1 - 3] = np.float32(0.0), np.float32(-0.0)
        assert t[3] == t[k - 1 - 3]
    assert bit_palindromic(t) == (form == "palindromic")
    return t


def name(kernel, k, d, fused):
    return f"{kernel}<{k},{d},{'true' if fused else 'false'},2,8,false,true,false,false>"


def n_in(k, d, nb):
    return (1024 * nb - 1) * d + k


_REFS = {}


def refs(oracle, k, d, fused, form):
    """inputs and oracle results of one (shape, rounding, taps) case, computed once"""
    key = (k, d, fused, form)
    if key not in _REFS:
        taps = make_taps(oracle, k, form)
        rng = np.random.default_rng(1000 * k + 10 * d + fused)
        r = {"taps": taps, "x": {}, "raw": {}, "chain": {}, "chain_u8": {}, "fir": {}}
        for nb in NBLOCKS:
            x = oracle.synth_iq(0x7AB5 + k + d + nb, 0, n_in(k, d, nb))
            raw = rng.integers(0, 256, 2 * n_in(k, d, nb), dtype=np.uint8)
            r["x"][nb], r["raw"][nb] = x, raw
            r["chain"][nb] = oracle.chain_fir_fft(x, taps, d, 1024, fused=fused)
            r["chain_u8"][nb] = oracle.chain_fir_fft(oracle.data_to_samples(raw), taps, d, 1024, fused=fused)
            r["fir"][nb] = oracle.fir(x, taps, d, fused=fused)
        _REFS[key] = r
    return _REFS[key]


def forms_of(k):
    return [f for f in FORMS if f != "quirk_nan" or k == 127]


CASES = [(k, d, fused, form) for k, d in SHAPES for fused in (True, False) for form in forms_of(k)]


@pytest.mark.parametrize("k,d,fused,form", CASES)
def test_chain_forms_bits(gpu, redio, oracle, k, d, fused, form):
    r = refs(oracle, k, d, fused, form)
    same = same_bits_or_nan if form == "quirk_nan" else same_bits
    chain = redio.Chain(r["taps"], d, 1024, fused=fused)
    assert chain.is_fused
    resident = name("chain_v4_kernel", k, d, fused)
    if form == "palindromic":
        assert chain.kernel_name == resident
    else:
        assert chain.kernel_name != resident
        assert chain.kernel_name == name("chain_v4_anytaps_kernel", k, d, fused)
    xs = {nb: gpu.from_numpy(r["x"][nb]).cuda() for nb in NBLOCKS}
    for nb in NBLOCKS:
        got = chain(xs[nb]).cpu().numpy()
        assert got.shape == (nb, 1024)
        assert same(got, r["chain"][nb]), f"cf32, {nb} blocks"
        got = chain.from_bytes(gpu.from_numpy(r["raw"][nb]).cuda()).cpu().numpy()
        assert same(got, r["chain_u8"][nb]), f"u8, {nb} blocks"
    outs = chain.enqueue_list([xs[nb] for nb in NBLOCKS])
    for nb, o in zip(NBLOCKS, outs):
        assert same(o.cpu().numpy(), r["chain"][nb]), f"list, message of {nb} blocks"


@pytest.mark.parametrize("k,d,fused,form", CASES)
def test_fir_forms_bits(gpu, redio, oracle, k, d, fused, form):
    """the stand-alone FIR at 1024 * nb outputs: whole blocks on the chain's data path for the shapes it is built for"""
    r = refs(oracle, k, d, fused, form)
    same = same_bits_or_nan if form == "quirk_nan" else same_bits
    fir = redio.Fir(r["taps"], d, complex_input=True, fused=fused)
    for nb in NBLOCKS:
        got = fir(gpu.from_numpy(r["x"][nb]).cuda()).cpu().numpy()
        assert got.shape == (1024 * nb,)
        assert same(got, r["fir"][nb]), f"{nb} blocks"


@pytest.mark.parametrize("fused", [True, False])
def test_two_plans_keep_their_forms(gpu, redio, oracle, fused):
    """one plan of each kind alive at once, launched alternately on one stream and through enqueue_list"""
    k, d = 127, 5
    ra, rb = refs(oracle, k, d, fused, "palindromic"), refs(oracle, k, d, fused, "ulp")
    a, b = redio.Chain(ra["taps"], d, 1024, fused=fused), redio.Chain(rb["taps"], d, 1024, fused=fused)
    assert a.kernel_name == name("chain_v4_kernel", k, d, fused)
    assert b.kernel_name == name("chain_v4_anytaps_kernel", k, d, fused)
    xa = {nb: gpu.from_numpy(ra["x"][nb]).cuda() for nb in NBLOCKS}
    xb = {nb: gpu.from_numpy(rb["x"][nb]).cuda() for nb in NBLOCKS}
    got = []
    for nb in NBLOCKS + NBLOCKS:
        got.append((a(xa[nb]), ra["chain"][nb]))
        got.append((b(xb[nb]), rb["chain"][nb]))
    la = a.enqueue_list([xa[nb] for nb in NBLOCKS])
    lb = b.enqueue_list([xb[nb] for nb in NBLOCKS])
    la2 = a.enqueue_list([xa[nb] for nb in NBLOCKS])
    gpu.cuda.synchronize()
    for g, w in got:
        assert same_bits(g.cpu().numpy(), w)
    for nb, oa, ob, oa2 in zip(NBLOCKS, la, lb, la2):
        assert same_bits(oa.cpu().numpy(), ra["chain"][nb])
        assert same_bits(ob.cpu().numpy(), rb["chain"][nb])
        assert same_bits(oa2.cpu().numpy(), ra["chain"][nb])
    assert not same_bits(ra["chain"][1], oracle.chain_fir_fft(ra["x"][1], rb["taps"], d, 1024, fused=fused)), "the two tap sets must differ in bits"


def test_designed_taps_keep_the_kernel_name(gpu, redio, oracle):
    taps = oracle.lpf_corrected(127, 0.08)
    assert bit_palindromic(taps)
    assert redio.Chain(taps, 5, 1024, fused=True).kernel_name == "chain_v4_kernel<127,5,true,2,8,false,true,false,false>"
