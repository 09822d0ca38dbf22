"""The integrated power spectrum (redio_pspec_*) on the MI355X: bit-exact against the restatement tests/pspec_ref.py on
the fused 1024-point kernel in its three launch modes and on the generic path; the chunk loop, the integration of a chain's spectra,
scratch and capture, carried history, special values and misuse."""
import ctypes as C

import numpy as np
import pytest

import pspec_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOT_RESERVED = -1, -6
SEED = 0x5EED0B5C


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def window_of(oracle, N, windowed):
    return oracle.lpf_corrected(N, 0.1) if windowed else None


def run(gpu, plan, xd):
    return plan(xd).cpu().numpy()


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 40])
def test_fused_bit_exact_in_every_mode(gpu, redio, oracle, K, windowed):
    """N = 1024: three rows and a partial row that is dropped, at no overlap, half overlap and a step that is no multiple of anything;
    one wave per row, one per segment with the fold pass, and auto (which splits here whenever K > 16) give the same bits"""
    N = 1024
    w = window_of(oracle, N, windowed)
    for step in (1024, 512, 1000):
        W, H = ref.shape(N, K, step)
        n = W + 2 * H + min(H - 1, 777)
        x = oracle.synth_iq(SEED + K, 0, n)
        want = ref.power_spectrum(x, N, K, step, w)
        assert want.shape == (3, N)
        plan = redio.PowerSpectrum(N, K, step, w)
        assert plan.is_fused and plan.nrows(n) == 3 and plan.nrows(W - 1) == 0 and plan.nrows(W) == 1 and plan.nrows(W + H) == 2
        xd = gpu.from_numpy(x).cuda()
        for mode in (0, 1, 2):
            plan.set_split(mode)
            got = run(gpu, plan, xd)
            assert got.shape == (3, N)
            assert np.array_equal(bits(got), bits(want)), (K, windowed, step, mode)
        assert np.array_equal(bits(run(gpu, plan, xd[: W + H])), bits(want[:2]))  # a shorter call on the same plan


GENERIC = [(6, 2, 6), (64, 33, 64), (1000, 5, 1000), (2048, 20, 2048), (4096, 4, 1000), (65536, 2, 65536)]


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("N,K,step", GENERIC)
def test_generic_bit_exact(gpu, redio, oracle, N, K, step, windowed):
    """every other size, two rows and a dropped partial row; 65536 is the two-pass transform (in place through its staging when rows are packed)"""
    w = window_of(oracle, N, windowed)
    W, H = ref.shape(N, K, step)
    n = W + H + min(H - 1, 5)
    x = oracle.synth_iq(SEED + N, 0, n)
    want = ref.power_spectrum(x, N, K, step, w)
    plan = redio.PowerSpectrum(N, K, step, w)
    assert not plan.is_fused and plan.nrows(n) == 2
    xd = gpu.from_numpy(x).cuda()
    for mode in (0, 2):
        plan.set_split(mode)
        assert np.array_equal(bits(run(gpu, plan, xd)), bits(want)), (N, K, step, windowed, mode)
    assert np.array_equal(bits(run(gpu, plan, xd[:W])), bits(want[:1]))


def test_generic_across_the_chunk_loop(gpu, redio, oracle):
    """N = 4096, K = 17: 2100 transforms are 123 rows of two segments; a pass through the scratch takes 128 segments = 64 rows.  The
    first row, the rows either side of the seam and the last against the restatement on their own windows."""
    N, K, ntr = 4096, 17, 2100
    rows = ntr // K
    chunk_rows = ((64 << 20) // (N * 8 * ref.SEG)) // 2
    assert rows == 123 and chunk_rows == 64
    x = redio.synth_iq(SEED + 1, 0, ntr * N)
    plan = redio.PowerSpectrum(N, K)
    assert plan.nrows(ntr * N) == rows
    y = plan(x)
    for r in (0, chunk_rows - 1, chunk_rows, rows - 1):
        want = ref.power_spectrum(oracle.synth_iq(SEED + 1, r * K * N, K * N), N, K)
        assert np.array_equal(bits(y[r].cpu().numpy()), bits(want[0])), r
    assert gpu.equal(plan(x), y)


def test_spectra_of_the_chain(gpu, redio, oracle):
    """redio_pspec_enqueue_spectra over redio_chain_enqueue's output: the 127-tap / 5 1024-point chain, 35 spectra, K = 17 -> 2 rows"""
    N, K, ntaps, D, nspec = 1024, 17, 127, 5, 35
    taps = oracle.lpf_corrected(ntaps, 0.08)
    x = oracle.synth_iq(SEED + 2, 0, (nspec * N - 1) * D + ntaps)
    X = oracle.chain_fir_fft(x, taps, D, N, False)
    assert X.shape == (nspec, N)
    want = ref.spectra(X, N, K)
    assert want.shape == (2, N)
    Xd = redio.Chain(taps, D, N, fused=False)(gpu.from_numpy(x).cuda())
    assert np.array_equal(bits(Xd.cpu().numpy().reshape(-1)), bits(X.reshape(-1)))
    for plan in (redio.PowerSpectrum(N, K), redio.PowerSpectrum(N, K, 512, oracle.lpf_corrected(N, 0.1))):  # window and step do not apply
        got = plan.spectra(Xd).cpu().numpy()
        assert np.array_equal(bits(got), bits(want))
    short = redio.PowerSpectrum(N, 3).spectra(Xd).cpu().numpy()  # K <= 16: the accumulate pass writes the rows
    assert np.array_equal(bits(short), bits(ref.spectra(X, N, 3))) and short.shape == (11, N)


def test_scratch_regrows_between_calls_on_one_plan(gpu, redio, oracle):
    """N = 96, K = 17 (two segments, the second of one transform), step 48, windowed, one plan: a 1-row call, the integration of 2 rows
    of spectra, a 9-row call that regrows the row scratch and the partials, 11 rows of spectra that regrow the partials once more, and
    the 1-row call again on scratch that is now larger than it needs"""
    N, K, step = 96, 17, 48
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    x = oracle.synth_iq(SEED + 8, 0, W + 8 * H)
    want = ref.power_spectrum(x, N, K, step, w)
    X = oracle.fft(oracle.synth_iq(SEED + 9, 0, 11 * K * N), N)
    want_spectra = ref.spectra(X, N, K)
    assert want.shape == (9, N) and want_spectra.shape == (11, N)
    plan = redio.PowerSpectrum(N, K, step, w)
    assert not plan.is_fused
    xd, Xd = gpu.from_numpy(x).cuda(), gpu.from_numpy(X).cuda()
    for rows, spectra_rows in ((1, 2), (9, 11), (1, None)):
        assert np.array_equal(bits(run(gpu, plan, xd[: W + (rows - 1) * H])), bits(want[:rows])), rows
        if spectra_rows:
            got = plan.spectra(Xd[: spectra_rows * K * N]).cpu().numpy()
            assert np.array_equal(bits(got), bits(want_spectra[:spectra_rows])), spectra_rows


@pytest.mark.parametrize("N,K,step,mode", [(1024, 17, 512, 1), (1024, 17, 512, 2), (1000, 5, 1000, 0), (64, 33, 64, 0)])
def test_reserve_then_capture_and_replay(gpu, redio, oracle, N, K, step, mode):
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    n = W + 3 * H
    x = oracle.synth_iq(SEED + 3, 0, n)
    want = ref.power_spectrum(x, N, K, step, w)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K, step, w)
    plan.set_split(mode)
    plan.reserve(n)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(xd, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count  # reserved: the enqueue allocated nothing


@pytest.mark.parametrize("N,K,mode", [(1024, 17, 2), (1000, 5, 0)])
def test_capture_needs_the_reserve(gpu, redio, oracle, N, K, mode):
    x = oracle.synth_iq(SEED + 4, 0, 2 * K * N)
    want = ref.power_spectrum(x, N, K)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K)
    plan.set_split(mode)
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(xd, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(plan(xd, out=out).cpu().numpy()), bits(want))  # the capture ended cleanly: the stream and the plan work on


@pytest.mark.parametrize("N,K,step", [(1024, 17, 512), (64, 33, 64)])
def test_stream_gives_the_one_shot_bits(gpu, redio, oracle, N, K, step):
    """messages of any length, a 1-sample one included: the concatenated rows are the one-shot plan's on the concatenated input"""
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    lens = [1, 7, W - 9, 1, H, W, W + 1, 3 * H + 5, 333, 2 * W + H - 1, 1, H - 1]
    x = redio.synth_iq(SEED + 5, 0, sum(lens))
    plan = redio.PowerSpectrum(N, K, step, w)
    whole = plan(x)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(ref.power_spectrum(x.cpu().numpy(), N, K, step, w)))
    s = redio.Stream(plan)
    for attempt in range(2):  # reset() starts over: the second pass repeats the first
        pos, outs, made = 0, [], 0
        for n in lens:
            expect = ref.nrows(pos + n, N, K, step) - made
            assert s.nout(n) == expect * N
            y = s(x[pos: pos + n])
            assert y.dtype == gpu.float32 and y.numel() == expect * N
            outs.append(y.clone())
            pos += n
            made += expect
            assert s.pending == pos - made * H
        assert gpu.equal(gpu.cat(outs), whole.reshape(-1)), (N, K, step, attempt)
        s.reset()
        assert s.pending == 0


def same_special(got, want):
    """tests/test_gpu_special_values.py: identical bits wherever the restatement's value is not a NaN, a NaN exactly where it has one"""
    g, w = np.ascontiguousarray(got).view(np.float32).reshape(-1), np.ascontiguousarray(want).view(np.float32).reshape(-1)
    wn = np.isnan(w)
    return g.shape == w.shape and np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


@pytest.mark.parametrize("finite", [True, False])
@pytest.mark.parametrize("N,K,mode", [(1024, 17, 1), (1024, 17, 2), (64, 33, 0)])
def test_special_values_in_one_transform(gpu, redio, oracle, N, K, mode, finite):
    """one transform of the middle row holds subnormals, signed zeros and large magnitudes (finite) and also +-inf and a NaN: NaNs exactly
    where the restatement has them, every other word bit-equal, and the rows that do not reach those samples unchanged"""
    clean = oracle.synth_iq(SEED + 6, 0, 3 * K * N)
    x = clean.copy()
    p = (K + K // 2) * N + N // 4  # inside transform K / 2 of row 1
    xs = x.view(np.float32)
    xs[2 * p: 2 * p + 8] = [1e-40, -0.0, -1.4e-45, 0.0, 3e38, -1e30, 2.0 ** -126, -1e-40]
    if not finite:
        xs[2 * p + 8: 2 * p + 11] = [np.inf, -np.inf, np.nan]
    plan = redio.PowerSpectrum(N, K)
    plan.set_split(mode)
    got = run(gpu, plan, gpu.from_numpy(x).cuda())
    with np.errstate(all="ignore"):
        want = ref.power_spectrum(x, N, K)
    assert same_special(got, want)
    assert finite or np.isnan(want[1]).any()
    base = run(gpu, plan, gpu.from_numpy(clean).cuda())
    for r in (0, 2):
        assert np.array_equal(bits(got[r]), bits(base[r]))


@pytest.mark.parametrize("N,K", [(1024, 4), (512, 3)])
def test_misuse(gpu, redio, oracle, N, K):
    L = redio.lib()
    plan = redio.PowerSpectrum(N, K)
    n = 2 * K * N
    x = redio.synth_iq(SEED + 7, 0, n + 2)
    out = gpu.full((2 * N + 2,), 7.0, dtype=gpu.float32, device="cuda")
    st = redio.current_stream()
    px, po = x.data_ptr(), out.data_ptr()
    assert px % 8 == 0 and po % 8 == 0
    for fn, count in ((L.redio_pspec_enqueue, n), (L.redio_pspec_enqueue_spectra, 2 * K)):
        assert fn(plan._h, C.c_void_p(px + 4), count, C.c_void_p(po), st) == ERR_ARG       # d_in on a 4-byte boundary
        assert fn(plan._h, C.c_void_p(px), count, C.c_void_p(po + 2), st) == ERR_ARG       # d_out on a 2-byte boundary
        assert fn(plan._h, C.c_void_p(px), count, C.c_void_p(px), st) == ERR_ARG           # in place
        assert fn(plan._h, C.c_void_p(px), count, C.c_void_p(px + 8 * (n // 2)), st) == ERR_ARG  # overlapping
        assert fn(plan._h, None, count, C.c_void_p(po), st) == ERR_ARG
        assert fn(plan._h, C.c_void_p(px), count, None, st) == ERR_ARG
        assert fn(None, C.c_void_p(px), count, C.c_void_p(po), st) == ERR_ARG
    assert L.redio_pspec_enqueue(plan._h, C.c_void_p(px), K * N - 1, C.c_void_p(po), st) == 0      # no whole row: nothing to do
    assert L.redio_pspec_enqueue_spectra(plan._h, C.c_void_p(px), K - 1, C.c_void_p(po), st) == 0
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and gpu.equal(x, redio.synth_iq(SEED + 7, 0, n + 2))             # nothing was launched
    assert L.redio_pspec_set_split(plan._h, 3) == ERR_ARG and L.redio_pspec_set_split(plan._h, -1) == ERR_ARG
    assert L.redio_pspec_reserve(None, n) == ERR_ARG
    with pytest.raises(redio.RedioError) as e:
        redio.PowerSpectrum(N, 0)
    assert e.value.code == ERR_ARG
