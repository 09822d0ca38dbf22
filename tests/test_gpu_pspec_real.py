"""The real-input integrated power spectrum (redio_pspec_real_*) on the MI355X: bit-exact against the restatement
tests/pspec_real_ref.py on the fused 2048-point kernel in its three launch modes and both load forms and on the generic path; the
chunk loop, the integration of redio_fftr's spectra, scratch and capture, carried history, special values and misuse."""
import ctypes as C

import numpy as np
import pytest

import fftr_ref
import pspec_real_ref as ref

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOT_RESERVED = -1, -6
SEED = 0x5EED0B5D


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def window_of(oracle, N, windowed):
    return oracle.lpf_corrected(N, 0.1) if windowed else None


def run(plan, xd):
    return plan(xd).cpu().numpy()


@pytest.mark.parametrize("step", [2048, 1024, 1000, 1001])
@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 40])
def test_fused_bit_exact_in_every_mode(gpu, redio, oracle, K, windowed, step):
    """N = 2048: three rows and a partial row that is dropped, at no overlap, half overlap, an even step that is no multiple of
    anything and an odd one (the 4-byte load form); one wave per row, one per segment with the fold pass, and auto (which splits
    here whenever K > 16) give the same bits, as do a base pointer one float into its allocation and a shorter call"""
    N, B = 2048, 1025
    w = window_of(oracle, N, windowed)
    W, H = ref.shape(N, K, step)
    n = W + 2 * H + min(H - 1, 777)
    x = oracle.synth_f32(SEED + K, 0, n)
    want = ref.power_spectrum(x, N, K, step, w)
    assert want.shape == (3, B)
    plan = redio.PowerSpectrumReal(N, K, step, w)
    assert plan.is_fused and plan.nbins == B
    assert plan.nrows(n) == 3 and plan.nrows(W - 1) == 0 and plan.nrows(W) == 1 and plan.nrows(W + H) == 2
    buf = gpu.empty(n + 1, dtype=gpu.float32, device="cuda")
    buf[:n] = gpu.from_numpy(x)
    xd = buf[:n]
    assert xd.data_ptr() % 8 == 0
    for mode in (0, 1, 2):
        plan.set_split(mode)
        got = run(plan, xd)
        assert got.shape == (3, B)
        assert np.array_equal(bits(got), bits(want)), (K, windowed, step, mode)
    assert np.array_equal(bits(run(plan, xd[: W + H])), bits(want[:2]))  # a shorter call on the same plan
    buf[1:] = gpu.from_numpy(x)
    xo = buf[1:]
    assert xo.data_ptr() % 8 == 4  # every transform starts on a 4-byte boundary only
    for mode in (1, 2):
        plan.set_split(mode)
        assert np.array_equal(bits(run(plan, xo)), bits(want)), (K, windowed, step, mode, "offset")


GENERIC = [(2, 3, 2), (6, 2, 6), (64, 33, 64), (1000, 5, 1000), (2050, 3, 2050), (4096, 4, 1000), (131072, 2, 131072)]


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("N,K,step", GENERIC)
def test_generic_bit_exact(gpu, redio, oracle, N, K, step, windowed):
    """every other even size, two rows and a dropped partial row; at 131072 M = 65536 is the two-pass transform.  Without a window
    at step == N the transform reads the caller's buffer; a base pointer one float into its allocation goes through the gather."""
    w = window_of(oracle, N, windowed)
    W, H = ref.shape(N, K, step)
    n = W + H + min(H - 1, 5)
    x = oracle.synth_f32(SEED + N, 0, n)
    want = ref.power_spectrum(x, N, K, step, w)
    plan = redio.PowerSpectrumReal(N, K, step, w)
    assert not plan.is_fused and plan.nrows(n) == 2 and plan.nbins == N // 2 + 1
    buf = gpu.empty(n + 1, dtype=gpu.float32, device="cuda")
    buf[:n] = gpu.from_numpy(x)
    xd = buf[:n]
    for mode in (0, 2):
        plan.set_split(mode)
        assert np.array_equal(bits(run(plan, xd)), bits(want)), (N, K, step, windowed, mode)
    assert np.array_equal(bits(run(plan, xd[:W])), bits(want[:1]))
    buf[1:] = gpu.from_numpy(x)
    assert np.array_equal(bits(run(plan, buf[1:])), bits(want)), "offset"


def test_scratch_regrows_between_calls_on_one_plan(gpu, redio, oracle):
    """N = 96, K = 17 (two segments, the second of one transform), step 48, windowed, one plan: a 1-row call, a 9-row call that regrows
    the row scratch, the spectrum scratch, the transform's own and the partials, and the 1-row call again"""
    N, K, step = 96, 17, 48
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    x = oracle.synth_f32(SEED + 8, 0, W + 8 * H)
    want = ref.power_spectrum(x, N, K, step, w)
    assert want.shape == (9, N // 2 + 1)
    plan = redio.PowerSpectrumReal(N, K, step, w)
    assert not plan.is_fused
    xd = gpu.from_numpy(x).cuda()
    for rows in (1, 9, 1):
        assert np.array_equal(bits(run(plan, xd[: W + (rows - 1) * H])), bits(want[:rows])), rows


def test_generic_across_the_chunk_loop(gpu, redio, oracle):
    """N = 4096, K = 17: a pass through the spectrum scratch takes (64 MiB) / (2049 * 8 * 16) = 255 segments, so the first seam falls
    between the two segments of row 127.  The first row, the rows either side of the seam and the last against the restatement
    on their own windows."""
    N, K, rows = 4096, 17, 131
    chunk_segs = (64 << 20) // (ref.nbins(N) * 8 * ref.SEG)
    assert chunk_segs == 255
    seam_row = chunk_segs // 2
    assert seam_row == 127
    x = redio.synth_f32(SEED + 1, 0, rows * K * N)
    plan = redio.PowerSpectrumReal(N, K)
    assert plan.nrows(rows * K * N) == rows
    y = plan(x)
    for r in (0, seam_row - 1, seam_row, seam_row + 1, rows - 1):
        want = ref.power_spectrum(oracle.synth_f32(SEED + 1, r * K * N, K * N), N, K)
        assert np.array_equal(bits(y[r].cpu().numpy()), bits(want[0])), r
    assert gpu.equal(plan(x), y)


@pytest.mark.parametrize("N", [2048, 64])
def test_spectra_of_the_real_transform(gpu, redio, oracle, N):
    """redio_pspec_real_enqueue_spectra over redio_fftr_enqueue's output: 35 spectra, K = 17 -> 2 rows, K = 3 -> 11; the restatement's
    bits, and those of enqueue on the same samples with no window at step == N"""
    nspec, B = 35, N // 2 + 1
    x = oracle.synth_f32(SEED + 2, 0, nspec * N)
    X = fftr_ref.fftr_rows(x, N)
    xd = gpu.from_numpy(x).cuda()
    Xd = redio.Fftr(N)(xd)
    assert np.array_equal(bits(Xd.cpu().numpy().reshape(-1)), bits(X.reshape(-1)))
    for K, rows in ((17, 2), (3, 11)):
        want = ref.spectra(X, N, K)
        assert want.shape == (rows, B)
        for plan in (redio.PowerSpectrumReal(N, K), redio.PowerSpectrumReal(N, K, N // 2, oracle.lpf_corrected(N, 0.1))):
            got = plan.spectra(Xd).cpu().numpy()  # window and step do not apply
            assert np.array_equal(bits(got), bits(want))
        assert np.array_equal(bits(run(redio.PowerSpectrumReal(N, K), xd)), bits(want))


@pytest.mark.parametrize("N,K,step,mode", [(2048, 17, 1024, 2), (1000, 5, 1000, 0), (64, 33, 64, 0)])
def test_reserve_then_capture_and_replay(gpu, redio, oracle, N, K, step, mode):
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    n = W + 3 * H
    x = oracle.synth_f32(SEED + 3, 0, n)
    want = ref.power_spectrum(x, N, K, step, w)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrumReal(N, K, step, w)
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


@pytest.mark.parametrize("N,K,mode", [(2048, 17, 2), (1000, 5, 0)])
def test_capture_needs_the_reserve(gpu, redio, oracle, N, K, mode):
    x = oracle.synth_f32(SEED + 4, 0, 2 * K * N)
    want = ref.power_spectrum(x, N, K)
    xd = gpu.from_numpy(x).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrumReal(N, K)
    plan.set_split(mode)
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(xd, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(plan(xd, out=out).cpu().numpy()), bits(want))  # the capture ended cleanly: the stream and the plan work on


@pytest.mark.parametrize("N,K,step,windowed", [(2048, 17, 1024, True), (64, 33, 64, False)])
def test_stream_gives_the_one_shot_bits(gpu, redio, oracle, N, K, step, windowed):
    """messages of any length, 1-sample and odd ones included: the concatenated rows are the one-shot plan's on the concatenated input"""
    w = window_of(oracle, N, windowed)
    B = N // 2 + 1
    W, H = ref.shape(N, K, step)
    lens = [1, 7, W - 9, 1, H, W, W + 1, 3 * H + 5, 333, 2 * W + H - 1, 1, H - 1]
    x = redio.synth_f32(SEED + 5, 0, sum(lens))
    plan = redio.PowerSpectrumReal(N, K, step, w)
    whole = plan(x)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(ref.power_spectrum(x.cpu().numpy(), N, K, step, w)))
    s = redio.Stream(plan)
    for attempt in range(2):  # reset() starts over: the second pass repeats the first
        pos, outs, made = 0, [], 0
        for n in lens:
            expect = ref.nrows(pos + n, N, K, step) - made
            assert s.nout(n) == expect * B
            y = s(x[pos: pos + n])
            assert y.dtype == gpu.float32 and y.numel() == expect * B
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
@pytest.mark.parametrize("N,K,mode", [(2048, 17, 1), (2048, 17, 2), (64, 33, 0)])
def test_special_values_in_one_transform(gpu, redio, oracle, N, K, mode, finite):
    """one transform of the middle row holds subnormals, signed zeros and large magnitudes (finite) and also +-inf and a NaN: NaNs exactly
    where the restatement has them, every other word bit-equal, and the rows that do not reach those samples unchanged"""
    clean = oracle.synth_f32(SEED + 6, 0, 3 * K * N)
    x = clean.copy()
    p = (K + K // 2) * N + N // 4  # inside transform K / 2 of row 1
    x[p: p + 8] = [1e-40, -0.0, -1.4e-45, 0.0, 3e38, -1e30, 2.0 ** -126, -1e-40]
    if not finite:
        x[p + 8: p + 11] = [np.inf, -np.inf, np.nan]
    plan = redio.PowerSpectrumReal(N, K)
    plan.set_split(mode)
    got = run(plan, gpu.from_numpy(x).cuda())
    with np.errstate(all="ignore"):
        want = ref.power_spectrum(x, N, K)
    assert same_special(got, want)
    assert finite or np.isnan(want[1]).any()
    base = run(plan, gpu.from_numpy(clean).cuda())
    for r in (0, 2):
        assert np.array_equal(bits(got[r]), bits(base[r]))


@pytest.mark.parametrize("N,K", [(2048, 4), (512, 3)])
def test_misuse(gpu, redio, oracle, N, K):
    L = redio.lib()
    plan = redio.PowerSpectrumReal(N, K)
    B = N // 2 + 1
    n = 2 * K * N
    x = redio.synth_f32(SEED + 7, 0, n + 4)
    out = gpu.full((2 * B + 2,), 7.0, dtype=gpu.float32, device="cuda")
    st = redio.current_stream()
    px, po = x.data_ptr(), out.data_ptr()
    assert px % 8 == 0 and po % 8 == 0
    assert L.redio_pspec_real_enqueue(plan._h, C.c_void_p(px + 2), n, C.c_void_p(po), st) == ERR_ARG    # d_in on a 2-byte boundary
    assert L.redio_pspec_real_enqueue_spectra(plan._h, C.c_void_p(px + 4), 2 * K, C.c_void_p(po), st) == ERR_ARG  # spectra: 8-byte aligned
    for fn, count, in_bytes in ((L.redio_pspec_real_enqueue, n, 4 * n), (L.redio_pspec_real_enqueue_spectra, 2 * K, 8 * 2 * K * B)):
        assert fn(plan._h, C.c_void_p(px), count, C.c_void_p(po + 2), st) == ERR_ARG       # d_out on a 2-byte boundary
        assert fn(plan._h, C.c_void_p(px), count, C.c_void_p(px), st) == ERR_ARG           # in place
        assert fn(plan._h, C.c_void_p(px), count, C.c_void_p(px + in_bytes - 8), st) == ERR_ARG  # overlapping
        assert fn(plan._h, None, count, C.c_void_p(po), st) == ERR_ARG
        assert fn(plan._h, C.c_void_p(px), count, None, st) == ERR_ARG
        assert fn(None, C.c_void_p(px), count, C.c_void_p(po), st) == ERR_ARG
    assert L.redio_pspec_real_enqueue(plan._h, C.c_void_p(px), K * N - 1, C.c_void_p(po), st) == 0      # no whole row: nothing to do
    assert L.redio_pspec_real_enqueue_spectra(plan._h, C.c_void_p(px), K - 1, C.c_void_p(po), st) == 0
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and gpu.equal(x, redio.synth_f32(SEED + 7, 0, n + 4))               # nothing was launched
    assert L.redio_pspec_real_set_split(plan._h, 3) == ERR_ARG and L.redio_pspec_real_set_split(plan._h, -1) == ERR_ARG
    assert L.redio_pspec_real_reserve(None, n) == ERR_ARG
    with pytest.raises(redio.RedioError) as e:
        redio.PowerSpectrumReal(N, 0)
    assert e.value.code == ERR_ARG
    with pytest.raises(redio.RedioError) as e:
        redio.PowerSpectrumReal(N + 1, K)  # odd
    assert e.value.code == ERR_ARG
    s = redio.Stream(plan)
    got = C.c_size_t(0)
    assert L.redio_pspec_real_stream_enqueue(s._h, C.c_void_p(px + 2), 8, C.c_void_p(po), C.byref(got), st) == ERR_ARG
    assert s.pending == 0
