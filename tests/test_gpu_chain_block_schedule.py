"""The chain kernel's block schedule (chain_v4.hip, chain_v4_body SCH): a wave loops over whole blocks of four sub-tiles whose place is a
compile-time fact, the transform's middle-stage twiddles come from a table in LDS, and a run's last block parks no further sub-tile.
(The form that also runs the transform of block b under the first FIR of block b + 1 measured no faster and is built only in the
measurement build; these cases hold for either.)  Bar: the bits of oracle.chain_fir_fft, with fmaf and with reference rounding, in
every case.

How long a wave's loop runs is the launcher's choice of blocks per wave (redio_chain_blocks_per_wave): one below 6 x the resident
waves, so the small sizes (1 ... 13 blocks) are runs of ONE block -- no next block anywhere.  Runs of 2, 3 and 4 blocks need launches
of tens of thousands of blocks; those cases read prefixes of one 2 GB device buffer, check sampled runs (the first, one in the
middle, the last full ones and the shorter last run) against the oracle -- a block depends on its own 1024 * D + K - D samples only --
and EVERY block against single launches of short messages (runs of one block, themselves checked against the oracle above)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL = (1, 2, 3, 4, 5, 8, 9, 13)
NMAX = max(SMALL)


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


_SMALL = {}


def small(oracle, k, d, fused, form="palindromic"):
    """input of NMAX blocks and its oracle spectra, once per case: a message of nb blocks is the prefix, its spectra the first nb rows"""
    key = (k, d, fused, form)
    if key not in _SMALL:
        taps = oracle.lpf_corrected(k, 0.08) if form == "palindromic" else ulp_taps(oracle, k)
        x = oracle.synth_iq(0xB10C + k + d, 0, n_in(k, d, NMAX))
        _SMALL[key] = (taps, x, oracle.chain_fir_fft(x, taps, d, 1024, fused=fused))
    return _SMALL[key]


@pytest.mark.parametrize("fused", [True, False])
def test_small_runs_bits(gpu, redio, oracle, fused):
    taps, x, want = small(oracle, 127, 5, fused)
    chain = redio.Chain(taps, 5, 1024, fused=fused)
    assert chain.is_fused and chain.kernel_name == f"chain_v4_kernel<127,5,{'true' if fused else 'false'},2,8,false,true,false,false>"
    dx = gpu.from_numpy(x).cuda()
    for nb in SMALL:
        got = chain(dx[: n_in(127, 5, nb)]).cpu().numpy()
        assert got.shape == (nb, 1024)
        assert same_bits(got, want[:nb]), f"{nb} blocks"


@pytest.mark.parametrize("fused", [True, False])
def test_small_offset_view_u8_anytaps_list(gpu, redio, oracle, fused):
    taps, x, want = small(oracle, 127, 5, fused)
    chain = redio.Chain(taps, 5, 1024, fused=fused)
    # a 16-byte-aligned offset view
    base = gpu.zeros(x.size + 2, dtype=gpu.complex64, device="cuda")
    view = base[2:]
    view.copy_(gpu.from_numpy(x))
    assert view.data_ptr() % 16 == 0 and view.data_ptr() != base.data_ptr()
    for nb in (5, 13):
        assert same_bits(chain(view[: n_in(127, 5, nb)]).cpu().numpy(), want[:nb]), f"offset view, {nb} blocks"
    # the receiver's u8 I/Q bytes
    raw = np.random.default_rng(0xB17E + fused).integers(0, 256, 2 * n_in(127, 5, NMAX), dtype=np.uint8)
    want_u8 = oracle.chain_fir_fft(oracle.data_to_samples(raw), taps, 5, 1024, fused=fused)
    draw = gpu.from_numpy(raw).cuda()
    for nb in (4, 5, 13):
        assert same_bits(chain.from_bytes(draw[: 2 * n_in(127, 5, nb)]).cpu().numpy(), want_u8[:nb]), f"u8, {nb} blocks"
    # taps one ulp off palindromic
    taps_u, xu, want_u = small(oracle, 127, 5, fused, "ulp")
    twin = redio.Chain(taps_u, 5, 1024, fused=fused)
    assert twin.kernel_name.startswith("chain_v4_anytaps_kernel<127,5,")
    dxu = gpu.from_numpy(xu).cuda()
    for nb in (1, 5, 13):
        assert same_bits(twin(dxu[: n_in(127, 5, nb)]).cpu().numpy(), want_u[:nb]), f"any taps, {nb} blocks"
    # a list launch of messages of 1, 2 and 5 blocks against one call per message
    dx = gpu.from_numpy(x).cuda()
    msgs = [dx[: n_in(127, 5, nb)] for nb in (1, 2, 5)]
    for c in (chain, twin):
        ref = want if c is chain else want_u
        src = msgs if c is chain else [dxu[: n_in(127, 5, nb)] for nb in (1, 2, 5)]
        outs = c.enqueue_list(src)
        singles = [c(m) for m in src]
        for nb, o, s in zip((1, 2, 5), outs, singles):
            assert same_bits(o.cpu().numpy(), s.cpu().numpy()), f"list against single call, {nb} blocks"
            assert same_bits(o.cpu().numpy(), ref[:nb]), f"list, {nb} blocks"


@pytest.mark.parametrize("k,d", [(63, 5), (127, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_small_other_shapes(gpu, redio, oracle, k, d, fused):
    taps, x, want = small(oracle, k, d, fused)
    chain = redio.Chain(taps, d, 1024, fused=fused)
    assert chain.is_fused
    assert same_bits(chain(gpu.from_numpy(x).cuda()).cpu().numpy(), want), f"({k}, {d}), {NMAX} blocks"


# ---- runs of two, three and four blocks: the loop goes round, the halo and the next sub-tile cross a transform ----------------------------------------------------

def first_size_with(chain, bpw):
    """smallest block count at which the launcher gives `bpw` blocks per wave (the rule is monotone in the block count)"""
    lo, hi = 1, 1 << 20
    assert chain.blocks_per_wave(hi) >= bpw
    while lo < hi:
        mid = (lo + hi) // 2
        if chain.blocks_per_wave(mid) >= bpw:
            hi = mid
        else:
            lo = mid + 1
    assert chain.blocks_per_wave(lo) == bpw
    return lo


@pytest.fixture(scope="module")
def big(gpu, redio, oracle):
    """one device stream for every long case: four blocks per wave plus a remainder run of three at (127, 5), plus the offset"""
    probe = redio.Chain(oracle.lpf_corrected(127, 0.08), 5, 1024, fused=True)
    nb4 = first_size_with(probe, 4)
    nb4 += 3 - nb4 % 4 if nb4 % 4 != 3 else 0
    assert probe.blocks_per_wave(nb4) == 4 and nb4 % 4 == 3
    x = redio.synth_iq(0xB16B10C, 0, n_in(127, 5, nb4) + 2)
    raw = gpu.randint(0, 256, (2 * n_in(127, 5, nb4),), dtype=gpu.uint8, device="cuda", generator=gpu.Generator(device="cuda").manual_seed(0xB16))
    yield {"x": x, "raw": raw, "nb4": nb4}
    del x, raw
    gpu.cuda.empty_cache()


def sampled_runs(nb, bpw):
    """block ranges [r0, r1): the first two runs, two in the middle, the last full runs and the shorter last run"""
    mid = (nb // bpw // 2) * bpw
    return [(0, 2 * bpw), (mid, mid + 2 * bpw), (nb - nb % bpw - 2 * bpw, nb)]


def check_long(gpu, oracle, chain, taps, k, d, fused, dx, nb, bpw, what, from_bytes=False):
    assert chain.blocks_per_wave(nb) == bpw, what
    assert chain.launch_waves(nb) == -(-nb // bpw), what
    n = n_in(k, d, nb)
    got = chain.from_bytes(dx[: 2 * n]) if from_bytes else chain(dx[:n])
    assert got.shape == (nb, 1024)
    for r0, r1 in sampled_runs(nb, bpw):
        lo, hi = r0 * 1024 * d, r0 * 1024 * d + n_in(k, d, r1 - r0)
        if from_bytes:
            xs = oracle.data_to_samples(dx[2 * lo: 2 * hi].cpu().numpy())
        else:
            xs = dx[lo:hi].cpu().numpy()
        want = oracle.chain_fir_fft(xs, taps, d, 1024, fused=fused)
        assert same_bits(got[r0:r1].cpu().numpy(), want), f"{what}: blocks {r0} ... {r1 - 1} differ from the oracle"
    # every block against launches of short messages: runs of one block
    step = 2048
    assert chain.blocks_per_wave(step) == 1
    for r0 in range(0, nb, step):
        r1 = min(r0 + step, nb)
        lo, hi = r0 * 1024 * d, r0 * 1024 * d + n_in(k, d, r1 - r0)
        part = chain.from_bytes(dx[2 * lo: 2 * hi]) if from_bytes else chain(dx[lo:hi])
        assert gpu.equal(part.view(gpu.int32), got[r0:r1].view(gpu.int32)), f"{what}: blocks {r0} ... {r1 - 1} differ from runs of one block"


@pytest.mark.parametrize("fused", [True, False])
def test_runs_of_four_plus_remainder(gpu, redio, oracle, big, fused):
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=fused)
    check_long(gpu, oracle, chain, taps, 127, 5, fused, big["x"], big["nb4"], 4, "four blocks per wave, last run of three")
    check_long(gpu, oracle, chain, taps, 127, 5, fused, big["x"][2:], big["nb4"], 4, "the same through a 16-byte offset view")


@pytest.mark.parametrize("fused", [True, False])
def test_runs_of_two_and_three(gpu, redio, oracle, big, fused):
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=fused)
    nb2, nb3 = first_size_with(chain, 2) + 1, first_size_with(chain, 3) + 2
    nb2 += 1 - nb2 % 2  # a last run of one
    check_long(gpu, oracle, chain, taps, 127, 5, fused, big["x"], nb2, 2, "two blocks per wave, last run of one")
    if nb3 % 3 == 0:
        nb3 += 1
    check_long(gpu, oracle, chain, taps, 127, 5, fused, big["x"], nb3, 3, "three blocks per wave, a shorter last run")


@pytest.mark.parametrize("fused", [True, False])
def test_long_u8_and_anytaps(gpu, redio, oracle, big, fused):
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=fused)
    check_long(gpu, oracle, chain, taps, 127, 5, fused, big["raw"], big["nb4"], 4, "u8, four blocks per wave", from_bytes=True)
    taps_u = ulp_taps(oracle, 127)
    twin = redio.Chain(taps_u, 5, 1024, fused=fused)
    assert twin.kernel_name.startswith("chain_v4_anytaps_kernel<127,5,")
    check_long(gpu, oracle, twin, taps_u, 127, 5, fused, big["x"], big["nb4"], 4, "any taps, four blocks per wave")


@pytest.mark.parametrize("k,d", [(63, 5), (127, 3)])
@pytest.mark.parametrize("fused", [True, False])
def test_long_other_shapes(gpu, redio, oracle, big, k, d, fused):
    """the other shapes at runs of four ((63, 5): a window of five read chunks, fewer than the transform has pieces)"""
    taps = oracle.lpf_corrected(k, 0.08)
    chain = redio.Chain(taps, d, 1024, fused=fused)
    nb = first_size_with(chain, 4) + 3
    if nb % 4 == 0:
        nb += 1
    assert n_in(k, d, nb) <= big["x"].numel()
    check_long(gpu, oracle, chain, taps, k, d, fused, big["x"], nb, 4, f"({k}, {d}), four blocks per wave")


def test_long_list_launch(gpu, redio, oracle, big):
    """a list whose total gives runs of four: messages of 1, 2 and 5 blocks beside a long one, against one call per message"""
    taps = oracle.lpf_corrected(127, 0.08)
    chain = redio.Chain(taps, 5, 1024, fused=True)
    x = big["x"]
    offs = [0, 7 * 5120, 11 * 5120, 20 * 5120]
    nbs = [1, 2, 5, big["nb4"] - 40]
    msgs = [x[o: o + n_in(127, 5, nb)] for o, nb in zip(offs, nbs)]
    outs = chain.enqueue_list(msgs)
    for nb, m, o in zip(nbs, msgs, outs):
        if nb <= 5:
            want = oracle.chain_fir_fft(m.cpu().numpy(), taps, 5, 1024, fused=True)
            assert same_bits(o.cpu().numpy(), want), f"list, message of {nb} blocks"
        assert gpu.equal(o.view(gpu.int32), chain(m).view(gpu.int32)), f"list against single call, {nb} blocks"
