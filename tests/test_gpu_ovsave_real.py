"""Overlap-save on real streams (redio_ovsave_real_*) on the MI355X: bit-exact against the restatement
tests/ovsave_real_ref.py and within the project's bound of the direct dsputils::convolve fold; the plan's scratch, capture, carried
history, special values and misuse."""
import ctypes as C

import numpy as np
import pytest

import ovsave_real_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOT_RESERVED = -1, -6
SEED = 0x5EED0105


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def taps_of(oracle, k):
    return oracle.lpf_corrected(k, 0.02) if k > 1 else np.array([0.75], np.float32)


def bound(taps, N):
    return 2e-6 * np.abs(taps).sum() * np.sqrt(np.log2(N)) + 1e-7  # tests/test_gpu_overlap_save.py:27


def check_prefixes(gpu, redio, oracle, N, k, counts, tail):
    """blocks are independent, so one restatement of the longest input serves every shorter one"""
    taps = taps_of(oracle, k)
    hop = ref.shape(k, N)[1]
    assert 0 <= tail < hop
    x = oracle.synth_f32(SEED, 0, N + (max(counts) - 1) * hop + tail)
    want = ref.overlap_save_real(x, taps, N)
    direct = oracle.convolve(x, taps)
    plan = redio.OverlapSaveReal(taps, N)
    assert plan.is_fused == (N == 2048) and plan.hop == hop
    xd = gpu.from_numpy(x).cuda()
    for nb in counts:
        n = N + (nb - 1) * hop + tail
        assert plan.nout(n) == nb * hop == ref.nout(n, k, N)
        got = plan(xd[:n]).cpu().numpy()
        assert len(got) == nb * hop
        assert np.array_equal(bits(got), bits(want[: nb * hop])), (N, k, nb)
        err = float(np.abs(got - direct[: nb * hop]).max())
        print(f"N={N} K={k} blocks={nb}: distance from the direct fold {err:.3g}, bound {bound(taps, N):.3g}")
        assert err <= bound(taps, N)
        assert np.array_equal(bits(plan(xd[:n]).cpu().numpy()), bits(got))  # the plan is reusable: a second call gives the same bits


@pytest.mark.parametrize("k", [1, 2, 127, 700, 2047])
def test_fused_bit_exact_and_close_to_direct(gpu, redio, oracle, k):
    """N = 2048: one block, a series of four and one past it, a workgroup of sixteen and one past it, 33; a ragged tail that fills no block"""
    hop = ref.shape(k, 2048)[1]
    check_prefixes(gpu, redio, oracle, 2048, k, (1, 4, 5, 16, 17, 33), min(hop - 1, 17))


@pytest.mark.parametrize("N,k", [(2, 1), (6, 3), (64, 1), (512, 63), (1000, 101), (4096, 1025), (4096, 4095), (131072, 127)])
def test_generic_bit_exact_and_close_to_direct(gpu, redio, oracle, N, k):
    """every other size, 1, 2 and 3 blocks; at 131072 the complex plan underneath is two-pass"""
    hop = ref.shape(k, N)[1]
    check_prefixes(gpu, redio, oracle, N, k, (1, 2, 3), min(hop - 1, 5))


def test_generic_across_the_chunk_loop(gpu, redio, oracle):
    """more blocks than one pass through the scratch (64 MiB of real rows = 4096 blocks of 4096): the first block, the blocks either side
    of the seam and the last against the restatement on their own windows"""
    N, k = 4096, 1025
    taps = taps_of(oracle, k)
    hop = ref.shape(k, N)[1]
    chunk = (64 << 20) // (N * 4)
    nblk = chunk + 2
    n = N + (nblk - 1) * hop + 7
    x = redio.synth_f32(SEED, 0, n)
    plan = redio.OverlapSaveReal(taps, N)
    assert plan.nout(n) == nblk * hop
    y = plan(x)
    for b in (0, chunk - 1, chunk, nblk - 1):
        want = ref.overlap_save_real(oracle.synth_f32(SEED, b * hop, N), taps, N)
        assert np.array_equal(bits(y[b * hop: (b + 1) * hop].cpu().numpy()), bits(want)), b
    assert gpu.equal(plan(x), y)


def test_short_input_and_even_tap_rule(gpu, redio, oracle):
    plan = redio.OverlapSaveReal(taps_of(oracle, 126), 2048)  # 126 taps count as 127
    assert plan.hop == 1922 and plan.nout(2047) == 0 and plan.nout(2048) == 1922
    assert plan(gpu.zeros(100, dtype=gpu.float32, device="cuda")).numel() == 0
    with pytest.raises(redio.RedioError) as e:
        redio.OverlapSaveReal(taps_of(oracle, 2048), 2048)  # ntaps == N: Ke = N + 1
    assert e.value.code == ERR_ARG


@pytest.mark.parametrize("N,k", [(2048, 127), (4096, 1025)])
def test_reserve_then_capture(gpu, redio, oracle, N, k):
    taps = taps_of(oracle, k)
    hop = ref.shape(k, N)[1]
    n = N + 4 * hop
    x = oracle.synth_f32(SEED + 1, 0, n)
    want = ref.overlap_save_real(x, taps, N)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(len(want), dtype=gpu.float32, device="cuda")
    plan = redio.OverlapSaveReal(taps, N)
    plan.reserve(n)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(xd, out=out)
    g.launch()
    gpu.cuda.synchronize()
    assert redio.lib().redio_malloc_count() == count  # reserved: the enqueue allocated nothing
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_capture_needs_the_reserve(gpu, redio, oracle):
    N, k = 1000, 101
    taps = taps_of(oracle, k)
    x = oracle.synth_f32(SEED + 2, 0, 3 * N)
    want = ref.overlap_save_real(x, taps, N)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(len(want), dtype=gpu.float32, device="cuda")
    plan = redio.OverlapSaveReal(taps, N)
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(xd, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(plan(xd, out=out).cpu().numpy()), bits(want))  # the capture ended cleanly: the stream and the plan work on


def lengths(N, hop, odd):
    if odd:
        return [1, 3, hop - 1, N + 1, 77, 3 * N + 5, 2 * hop + 1, 999, hop + 1, 5, N - 1, 4 * hop - 1]
    return [1, 7, hop - 1, hop, N, N + 1, 3 * N + 5] * 2


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("N,k", [(2048, 127), (512, 64)])
def test_stream_gives_the_one_shot_bits(gpu, redio, oracle, N, k, odd):
    """messages of any length: the concatenated outputs are the one-shot plan's on the concatenated input"""
    taps = taps_of(oracle, k)
    hop = ref.shape(k, N)[1]
    lens = lengths(N, hop, odd)
    assert not odd or all(n % 2 for n in lens)
    x = redio.synth_f32(SEED + 3, 0, sum(lens))
    plan = redio.OverlapSaveReal(taps, N)
    whole = plan(x)
    host = x.cpu().numpy()
    nb = min(3, whole.numel() // hop)
    assert np.array_equal(bits(whole[: nb * hop].cpu().numpy()), bits(ref.overlap_save_real(host[: N + (nb - 1) * hop], taps, N)))
    s = redio.Stream(plan)
    for attempt in range(2):  # reset() starts over: the second pass repeats the first
        pos, outs, made = 0, [], 0
        for n in lens:
            expect = ref.nout(pos + n, k, N) - made
            assert s.nout(n) == expect
            y = s(x[pos: pos + n])
            assert y.numel() == expect
            outs.append(y.clone())
            pos += n
            made += expect
            assert s.pending == pos - (made // hop) * hop
        assert gpu.equal(gpu.cat(outs), whole), (N, k, odd, attempt)
        s.reset()
        assert s.pending == 0


def same_special(got, want):
    g, w = np.ascontiguousarray(got).view(np.float32).reshape(-1), np.ascontiguousarray(want).view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


@pytest.mark.parametrize("finite", [True, False])
@pytest.mark.parametrize("N,k", [(2048, 127), (512, 63)])
def test_special_values_in_one_block(gpu, redio, oracle, N, k, finite):
    """the middle block of five holds a subnormal and -0 (finite) and also +-inf and a NaN (not finite): NaNs exactly where the restatement
    has them, every other word bit-equal, and the blocks that do not reach those samples unchanged"""
    taps = taps_of(oracle, k)
    hop = ref.shape(k, N)[1]
    clean = oracle.synth_f32(SEED + 4, 0, N + 4 * hop)
    x = clean.copy()
    p = 2 * hop + N // 2  # inside block 2 only: block 1 ends at hop + N <= p, block 3 starts at 3 hop > p + 8
    assert hop + N <= p and p + 8 < 3 * hop
    x[p: p + 3] = [1e-40, -0.0, -1.4e-45]
    if not finite:
        x[p + 4: p + 7] = [np.inf, -np.inf, np.nan]
    plan = redio.OverlapSaveReal(taps, N)
    got = plan(gpu.from_numpy(x).cuda()).cpu().numpy()
    want = ref.overlap_save_real(x, taps, N)
    assert same_special(got, want)
    assert finite or np.isnan(want[2 * hop: 3 * hop]).any()
    base = plan(gpu.from_numpy(clean).cuda()).cpu().numpy()
    for b in (0, 1, 3, 4):
        assert np.array_equal(bits(got[b * hop: (b + 1) * hop]), bits(base[b * hop: (b + 1) * hop]))


@pytest.mark.parametrize("N,k", [(2048, 127), (512, 63)])
def test_misuse(gpu, redio, oracle, N, k):
    L = redio.lib()
    plan = redio.OverlapSaveReal(taps_of(oracle, k), N)
    n = N + plan.hop
    x = redio.synth_f32(SEED + 5, 0, n + 2)
    out = gpu.full((2 * plan.hop + 2,), 7.0, dtype=gpu.float32, device="cuda")
    st = redio.current_stream()
    px, po = x.data_ptr(), out.data_ptr()
    assert px % 8 == 0 and po % 8 == 0
    assert L.redio_ovsave_real_enqueue(plan._h, C.c_void_p(px + 4), n, C.c_void_p(po), st) == ERR_ARG       # d_in on a 4-byte boundary
    assert L.redio_ovsave_real_enqueue(plan._h, C.c_void_p(px), n, C.c_void_p(po + 4), st) == ERR_ARG       # d_out on a 4-byte boundary
    assert L.redio_ovsave_real_enqueue(plan._h, C.c_void_p(px), n, C.c_void_p(px), st) == ERR_ARG           # in place
    assert L.redio_ovsave_real_enqueue(plan._h, C.c_void_p(px), n, C.c_void_p(px + 8 * (n // 4)), st) == ERR_ARG  # overlapping
    assert L.redio_ovsave_real_enqueue(plan._h, None, n, C.c_void_p(po), st) == ERR_ARG
    assert L.redio_ovsave_real_enqueue(plan._h, C.c_void_p(px), n, None, st) == ERR_ARG
    assert L.redio_ovsave_real_enqueue(None, C.c_void_p(px), n, C.c_void_p(po), st) == ERR_ARG
    assert L.redio_ovsave_real_enqueue(plan._h, C.c_void_p(px), N - 1, C.c_void_p(po), st) == 0             # no whole block: nothing to do
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and gpu.equal(x, redio.synth_f32(SEED + 5, 0, n + 2))                   # nothing was launched
    assert L.redio_ovsave_real_reserve(None, n) == ERR_ARG
