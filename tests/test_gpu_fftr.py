"""The real-input transform on the MI355X (redio_fftr_*, kiss_fftr / kiss_fftri): bit for bit against tests/fftr_ref.py."""
import ctypes as C

import numpy as np
import pytest

import fftr_ref

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_NOT_RESERVED = -1, -6
GENERIC = [2, 4, 6, 8, 10, 30, 128, 200, 512, 1000, 4096, 8192, 32768, 131072]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def host(t):
    return t.cpu().numpy()


_cache = {}


def case(oracle, N, rows, inverse, seed=0):
    """(input rows, expected output rows) of `rows` transforms, computed once per shape and never modified."""
    key = (N, rows, inverse, seed)
    if key not in _cache:
        if inverse:
            x = oracle.synth_iq(0x1F00 + N + seed, 0, rows * (N // 2 + 1))
            want = fftr_ref.fftri_rows(x, N)
        else:
            x = oracle.synth_f32(0x1E00 + N + seed, 0, rows * N)
            want = fftr_ref.fftr_rows(x, N)
        x.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (x, want)
    return _cache[key]


def nan_buf(gpu, n, dtype):
    """n elements whose every 32-bit word is a NaN (both parts of a complex element)."""
    if dtype == gpu.complex64:
        return gpu.view_as_complex(gpu.full((n, 2), float("nan"), dtype=gpu.float32, device="cuda"))
    return gpu.full((n,), float("nan"), dtype=dtype, device="cuda")


def guarded(gpu, n, dtype):
    """A NaN-filled buffer with 8 guard elements on each side of n."""
    buf = nan_buf(gpu, n + 16, dtype)
    return buf, buf[8 : 8 + n]


def guards_untouched(buf):
    h = host(buf)
    return bool(np.isnan(h[:8].view(np.float32)).all() and np.isnan(h[-8:].view(np.float32)).all())


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("nbatch", [1, 3, 4, 5, 16, 17])
def test_fused_2048(redio, gpu, oracle, nbatch, inverse):
    N = 2048
    x, want = case(oracle, N, 17, inverse)
    nin, nout = (N // 2 + 1, N) if inverse else (N, N // 2 + 1)
    plan = redio.Fftr(N, inverse)
    assert plan.is_fused
    buf, out = guarded(gpu, nbatch * nout, gpu.float32 if inverse else gpu.complex64)
    plan(gpu.from_numpy(x[: nbatch * nin].copy()).cuda(), out=out)
    got = host(out).reshape(nbatch, nout)
    assert np.array_equal(bits(got), bits(want[:nbatch]))  # packed rows at odd batch index are the 8-byte-aligned ones
    assert guards_untouched(buf)


@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("N", GENERIC)
def test_generic_sizes(redio, gpu, oracle, N, inverse):
    nin, nout = (N // 2 + 1, N) if inverse else (N, N // 2 + 1)
    big = N == 131072
    x, want = case(oracle, N, 2 if big else 3, inverse)
    plan = redio.Fftr(N, inverse)
    assert not plan.is_fused
    for nbatch in ((1, 2) if big else (1, 3)):
        buf, out = guarded(gpu, nbatch * nout, gpu.float32 if inverse else gpu.complex64)
        plan(gpu.from_numpy(x[: nbatch * nin].copy()).cuda(), out=out)
        assert np.array_equal(bits(host(out).reshape(nbatch, nout)), bits(want[:nbatch])), (N, nbatch)
        assert guards_untouched(buf)


@pytest.mark.parametrize("N,in_stride,out_strides", [(2048, 2, (1025, 1026, 1100)), (2048, 512, (1025, 1026, 1100)), (2048, 2048, (1025, 1026, 1100)),
                                                     (2048, 2050, (1025, 1026, 1100)), (200, 50, (101, 104))])
def test_strided_forward(redio, gpu, oracle, N, in_stride, out_strides):
    nbatch, nb = 9, N // 2 + 1
    x = oracle.synth_f32(0x2A00 + in_stride, 0, (nbatch - 1) * in_stride + N)
    want = np.stack([fftr_ref.fftr(x[b * in_stride : b * in_stride + N]) for b in range(nbatch)])
    plan = redio.Fftr(N)
    xd = gpu.from_numpy(x).cuda()
    for out_stride in out_strides:
        out = nan_buf(gpu, (nbatch - 1) * out_stride + nb, gpu.complex64)
        plan.strided(xd, nbatch, in_stride, out_stride, out=out)
        h = host(out)
        for b in range(nbatch):
            assert np.array_equal(bits(h[b * out_stride : b * out_stride + nb]), bits(want[b])), (in_stride, out_stride, b)
            if b + 1 < nbatch:  # the gap between rows stays as it was
                assert np.isnan(h[b * out_stride + nb : (b + 1) * out_stride].view(np.float32)).all()


@pytest.mark.parametrize("N,in_stride,out_strides", [(2048, 1030, (2048, 2052)), (200, 110, (200, 204))])
def test_strided_inverse(redio, gpu, oracle, N, in_stride, out_strides):
    nbatch, nb = 5, N // 2 + 1
    f = oracle.synth_iq(0x2B00 + N, 0, (nbatch - 1) * in_stride + nb)
    want = np.stack([fftr_ref.fftri(f[b * in_stride : b * in_stride + nb]) for b in range(nbatch)])
    plan = redio.Fftr(N, inverse=True)
    fd = gpu.from_numpy(f).cuda()
    for out_stride in out_strides:
        out = nan_buf(gpu, (nbatch - 1) * out_stride + N, gpu.float32)
        plan.strided(fd, nbatch, in_stride, out_stride, out=out)
        h = host(out)
        for b in range(nbatch):
            assert np.array_equal(bits(h[b * out_stride : b * out_stride + N]), bits(want[b])), (out_stride, b)
            if b + 1 < nbatch:
                assert np.isnan(h[b * out_stride + N : (b + 1) * out_stride]).all()


def test_nan_frame_stays_in_its_frame(redio, gpu, oracle):
    N = 2048
    x, _ = case(oracle, N, 17, False)
    x = x[: 8 * N].copy()
    plan = redio.Fftr(N)
    clean = host(plan(gpu.from_numpy(x).cuda())).reshape(8, -1)
    x[5 * N : 6 * N] = np.nan
    dirty = host(plan(gpu.from_numpy(x).cuda())).reshape(8, -1)
    keep = [b for b in range(8) if b != 5]
    assert np.array_equal(bits(dirty[keep]), bits(clean[keep]))
    assert np.isnan(dirty[5].view(np.float32)).any()


@pytest.mark.parametrize("N", [2048, 1000])
def test_agrees_with_the_complex_transform(redio, gpu, oracle, N):
    x, _ = case(oracle, N, 3, False)
    xd = gpu.from_numpy(x.copy()).cuda()
    real = host(redio.Fftr(N)(xd)).reshape(3, -1).astype(np.complex128)
    full = host(redio.Fft(N)(xd.to(gpu.complex64))).reshape(3, N)[:, : N // 2 + 1].astype(np.complex128)
    err = np.linalg.norm(real - full) / np.linalg.norm(full)
    print(f"N={N}: relative L2 against the complex transform {err:.3g}")
    assert err <= 2e-6


def test_misuse(redio, gpu):
    L = redio.lib()
    h = C.c_void_p()
    for nfft in (7, 1, 0, -2):
        assert L.redio_fftr_create(C.byref(h), nfft, 0) == ERR_ARG and not h.value
    assert L.redio_fftr_create(None, 64, 0) == ERR_ARG
    st = redio.current_stream()
    for N in (2048, 64):
        nb = N // 2 + 1
        fwd, inv = redio.Fftr(N), redio.Fftr(N, inverse=True)
        t = nan_buf(gpu, 4 * N, gpu.float32)
        f = nan_buf(gpu, 4 * nb + 8, gpu.complex64)
        tp, fp = t.data_ptr(), f.data_ptr()
        bad = [
            (fwd, None, fp, 1, N, nb), (fwd, tp, None, 1, N, nb), (fwd, tp, tp, 1, N, nb),  # NULL, aliasing
            (fwd, tp, fp, 2, 0, nb), (fwd, tp, fp, 2, -N, nb), (fwd, tp, fp, 2, N - 1, nb),  # the real-side stride is positive and even
            (fwd, tp, fp, 2, N, nb - 1), (fwd, tp + 4, fp, 1, N, nb), (fwd, tp, fp + 4, 1, N, nb),  # rows overlap; not 8-byte aligned
            (inv, fp, tp, 2, nb, N - 2), (inv, fp, tp, 2, nb, N + 1), (inv, fp, tp, 2, 0, N), (inv, fp, None, 1, nb, N),
        ]
        for plan, a, b, n, si, so in bad:
            assert L.redio_fftr_enqueue_strided(plan._h, a, b, n, si, so, st) == ERR_ARG, (N, n, si, so)
        assert L.redio_fftr_enqueue(fwd._h, None, fp, 1, st) == ERR_ARG and L.redio_fftr_enqueue(fwd._h, tp, tp, 1, st) == ERR_ARG
        assert L.redio_fftr_enqueue(None, tp, fp, 1, st) == ERR_ARG
        assert L.redio_fftr_enqueue(fwd._h, None, None, 0, st) == 0 and L.redio_fftr_enqueue_strided(inv._h, fp, tp, 0, nb, N, st) == 0
        gpu.cuda.synchronize()
        assert np.isnan(host(t)).all() and np.isnan(host(f).view(np.float32)).all()  # nothing was launched


def test_reserve_then_no_allocation(redio, gpu, oracle):
    N = 1000
    x, want = case(oracle, N, 3, False)
    plan = redio.Fftr(N)
    plan.reserve(3)
    xd = gpu.from_numpy(x.copy()).cuda()
    out = gpu.empty(3 * (N // 2 + 1), dtype=gpu.complex64, device="cuda")
    before = redio.lib().redio_malloc_count()
    for _ in range(3):
        plan(xd, out=out)
    assert redio.lib().redio_malloc_count() == before
    assert np.array_equal(bits(host(out).reshape(3, -1)), bits(want))


def test_capture_needs_the_reserve(redio, gpu, oracle):
    N = 1000
    x, want = case(oracle, N, 3, False)
    xd = gpu.from_numpy(x.copy()).cuda()
    out = gpu.zeros(3 * (N // 2 + 1), dtype=gpu.complex64, device="cuda")
    plan = redio.Fftr(N)
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan(xd, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    plan.reserve(3)
    g2 = redio.Graph()
    with g2:
        plan(xd, out=out)
    g2.launch()
    gpu.cuda.synchronize()
    assert np.array_equal(bits(host(out).reshape(3, -1)), bits(want))
    fused = redio.Fftr(2048)  # the fused size needs no reserve
    x2, want2 = case(oracle, 2048, 17, False)
    d2 = gpu.from_numpy(x2[: 3 * 2048].copy()).cuda()
    out2 = gpu.zeros(3 * 1025, dtype=gpu.complex64, device="cuda")
    g3 = redio.Graph()
    with g3:
        fused(d2, out=out2)
    g3.launch()
    gpu.cuda.synchronize()
    assert np.array_equal(bits(host(out2).reshape(3, -1)), bits(want2[:3]))


@pytest.mark.parametrize("N", [2048, 30])
def test_drop_in(redio, gpu, oracle, N):
    x, want = case(oracle, N, 3, False)
    g, gwant = case(oracle, N, 3, True)
    fwd, inv = redio.kissfft.RealCfg(N), redio.kissfft.RealCfg(N, 1)
    assert np.array_equal(bits(fwd(x[:N])), bits(want[0]))
    assert np.array_equal(bits(inv(g[: N // 2 + 1])), bits(gwant[0]))
    # a forward call on an inverse cfg: the published code exits; here the output is poisoned and the process goes on
    K = redio.kisslib()
    out = np.zeros(N // 2 + 1, np.complex64)
    src = np.ascontiguousarray(x[:N])
    K.kiss_fftr(inv._cfg, src.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert np.isnan(out.view(np.float32)).all()
    tout = np.zeros(N, np.float32)
    K.kiss_fftri(fwd._cfg, np.ascontiguousarray(g[: N // 2 + 1]).ctypes.data_as(C.c_void_p), tout.ctypes.data_as(C.c_void_p))
    assert np.isnan(tout).all()
    assert np.array_equal(bits(fwd(x[N : 2 * N])), bits(want[1]))  # and the cfg still works
    fwd.close()
    inv.close()


def test_drop_in_placement(redio, gpu, oracle):
    K = redio.kisslib()
    N = 30
    need = C.c_size_t(0)
    assert K.kiss_fftr_alloc(N, 0, None, C.byref(need)) is None and need.value > 0
    arena = C.create_string_buffer(need.value + 3)
    base = C.addressof(arena) + 3  # any alignment of mem is accepted
    n2 = C.c_size_t(need.value)
    cfg = K.kiss_fftr_alloc(N, 0, C.c_void_p(base), C.byref(n2))
    assert cfg and base <= cfg < base + need.value and n2.value == need.value
    x, want = case(oracle, N, 3, False)
    out = np.zeros(N // 2 + 1, np.complex64)
    K.kiss_fftr(cfg, np.ascontiguousarray(x[:N]).ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
    assert np.array_equal(bits(out), bits(want[0]))
    K.kiss_fftr_free(cfg)
    small = C.c_size_t(need.value - 1)
    assert K.kiss_fftr_alloc(N, 0, C.c_void_p(base), C.byref(small)) is None and small.value == need.value


def test_randomised(redio, gpu, oracle):
    rng = np.random.default_rng(0xFF7A)
    smooth = [n for n in range(2, 4097, 2) if _smooth(n // 2)]
    rough = [14, 22, 26, 34, 442, 2002, 3094]
    plans = {}
    for draw in range(40):
        N = int(rng.choice(rough)) if draw % 8 == 7 else int(rng.choice(smooth))
        nbatch, inverse = int(rng.integers(1, 10)), bool(rng.integers(0, 2))
        nin, nout = (N // 2 + 1, N) if inverse else (N, N // 2 + 1)
        if inverse:
            x = oracle.synth_iq(0x3000 + draw, 0, nbatch * nin)
            want = fftr_ref.fftri_rows(x, N)
        else:
            x = oracle.synth_f32(0x3000 + draw, 0, nbatch * nin)
            want = fftr_ref.fftr_rows(x, N)
        plan = plans.setdefault((N, inverse), redio.Fftr(N, inverse))
        got = host(plan(gpu.from_numpy(x).cuda())).reshape(nbatch, nout)
        assert np.array_equal(bits(got), bits(want)), (draw, N, nbatch, inverse)


def _smooth(m):
    for p in (2, 3, 5):
        while m % p == 0:
            m //= p
    return m == 1
