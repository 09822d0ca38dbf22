"""The integrated power spectrum from the receiver's u8 I/Q bytes (redio_pspec_enqueue_u8) on the MI355X: bit for bit
pspec_ref.power_spectrum(oracle.data_to_samples(bytes), ...) on the fused 1024-point kernel in its three launch modes and on the
generic path, and the same bits as the on-device two-call path; byte buffers that are only 2-byte aligned, every byte pair, the chunk
loop, scratch and capture, carried history and misuse.  Everything is compared as uint32 bit patterns."""
import ctypes as C

import numpy as np
import pytest

import pspec_ref as ref

pytestmark = pytest.mark.gpu

OK, ERR_ARG, ERR_NOT_RESERVED = 0, -1, -6
SEED = 0x5EED0B5C


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def window_of(oracle, N, windowed):
    return oracle.lpf_corrected(N, 0.1) if windowed else None


def checker(oracle, raw, N, K, step, w):
    return ref.power_spectrum(oracle.data_to_samples(raw), N, K, step, w)


def at_offset(gpu, raw, off):
    """the bytes on the device, starting `off` bytes into a larger allocation"""
    big = gpu.zeros(raw.size + 16, dtype=gpu.uint8, device="cuda")
    assert big.data_ptr() % 16 == 0
    view = big[off: off + raw.size]
    view.copy_(gpu.from_numpy(raw))
    assert view.data_ptr() == big.data_ptr() + off
    return view


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("K", [1, 3, 16, 17, 40])
def test_fused_bit_exact_in_every_mode(gpu, redio, oracle, K, windowed):
    """N = 1024: three rows and a dropped partial row at no overlap, half overlap and a step that is a multiple of nothing; one wave
    per row, one per segment with the fold pass, and auto give the checker's bits, and so does data_to_samples + __call__ on the device"""
    from libredio_amd import bitfount
    N = 1024
    w = window_of(oracle, N, windowed)
    for step in (1024, 512, 1000):
        W, H = ref.shape(N, K, step)
        n = W + 2 * H + min(H - 1, 777)
        raw = random_bytes(SEED + K, 2 * n)
        want = checker(oracle, raw, N, K, step, w)
        assert want.shape == (3, N)
        plan = redio.PowerSpectrum(N, K, step, w)
        assert plan.is_fused
        rd = gpu.from_numpy(raw).cuda()
        for mode in (0, 1, 2):
            plan.set_split(mode)
            got = plan.u8(rd).cpu().numpy()
            assert got.shape == (3, N)
            assert np.array_equal(bits(got), bits(want)), (K, windowed, step, mode)
        two = plan(bitfount.data_to_samples(rd)).cpu().numpy()
        assert np.array_equal(bits(two), bits(want)), (K, windowed, step)
        assert np.array_equal(bits(plan.u8(rd[: 2 * (W + H)]).cpu().numpy()), bits(want[:2]))  # a shorter call on the same plan


@pytest.mark.parametrize("off", [2, 6])
def test_fused_on_a_2_byte_aligned_buffer(gpu, redio, oracle, off):
    """the byte buffer starts at byte 2 or 6 of its allocation: 2-byte aligned, not 4-, 8- or 16-byte aligned; step 1000, K = 17, windowed"""
    N, K, step = 1024, 17, 1000
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    raw = random_bytes(SEED + 100 + off, 2 * (W + 2 * H + 777))
    want = checker(oracle, raw, N, K, step, w)
    plan = redio.PowerSpectrum(N, K, step, w)
    rd = at_offset(gpu, raw, off)
    assert rd.data_ptr() % 4 == 2
    for mode in (1, 2):
        plan.set_split(mode)
        assert np.array_equal(bits(plan.u8(rd).cpu().numpy()), bits(want)), (off, mode)


def test_all_byte_pairs(gpu, redio, oracle):
    """the 65 536 (I, Q) pairs in order are 64 transforms of 1024; K = 16 gives 4 rows"""
    pairs = np.stack(np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij"), axis=-1).reshape(-1)
    assert pairs.size == 2 * 65536 and tuple(pairs[:4]) == (0, 0, 0, 1)
    want = checker(oracle, pairs, 1024, 16, 1024, None)
    assert want.shape == (4, 1024)
    got = redio.PowerSpectrum(1024, 16).u8(gpu.from_numpy(pairs).cuda()).cpu().numpy()
    assert np.array_equal(bits(got), bits(want))


# (15, 3, 7): an odd size, where a lane step of the gather straddles two rows and a one-row call has an odd element count
GENERIC = [(6, 2, 6), (64, 33, 64), (1000, 5, 1000), (2048, 20, 2048), (4096, 4, 1000), (65536, 2, 65536), (15, 3, 7)]


@pytest.mark.parametrize("windowed", [False, True])
@pytest.mark.parametrize("N,K,step", GENERIC)
def test_generic_bit_exact(gpu, redio, oracle, N, K, step, windowed):
    """every other size, two rows and a dropped partial row, from a buffer at byte offset 2.  Un-windowed at step = N the plan's cf32
    path reads the caller's buffer and never packs, but the u8 call packs and transforms in place: at 65536 that transform stages.
    2048 and 4096 go through the one-wave transforms that convert and window at their own load (step 1000 at 4096: strided)."""
    w = window_of(oracle, N, windowed)
    W, H = ref.shape(N, K, step)
    n = W + H + min(H - 1, 5)
    raw = random_bytes(SEED + N, 2 * n)
    want = checker(oracle, raw, N, K, step, w)
    plan = redio.PowerSpectrum(N, K, step, w)
    assert not plan.is_fused and plan.nrows(n) == 2
    rd = at_offset(gpu, raw, 2)
    for mode in (0, 2):
        plan.set_split(mode)
        assert np.array_equal(bits(plan.u8(rd).cpu().numpy()), bits(want)), (N, K, step, windowed, mode)
    assert np.array_equal(bits(plan.u8(rd[: 2 * W]).cpu().numpy()), bits(want[:1]))


@pytest.mark.parametrize("N", [96, 2048])
def test_scratch_regrows_between_calls_on_one_plan(gpu, redio, oracle, N):
    """K = 17 (two segments, the second of one transform), step N / 2, windowed, one plan, at a size that gathers and transforms in
    place (96) and at one whose transform reads the bytes itself (2048): a 1-row call, the integration of 2 rows of spectra, a 9-row
    call that regrows the row scratch and the partials, the cf32 entry on the same samples, 11 rows of spectra that regrow the
    partials once more, and the 1-row call again"""
    from libredio_amd import bitfount
    K, step = 17, N // 2
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    raw = random_bytes(SEED + 8 + N, 2 * (W + 8 * H))
    want = checker(oracle, raw, N, K, step, w)
    X = oracle.fft(oracle.synth_iq(SEED + 9, 0, 11 * K * N), N)
    want_spectra = ref.spectra(X, N, K)
    assert want.shape == (9, N) and want_spectra.shape == (11, N)
    plan = redio.PowerSpectrum(N, K, step, w)
    assert not plan.is_fused
    rd, Xd = gpu.from_numpy(raw).cuda(), gpu.from_numpy(X).cuda()
    for rows, spectra_rows in ((1, 2), (9, 11), (1, None)):
        nbytes = 2 * (W + (rows - 1) * H)
        assert np.array_equal(bits(plan.u8(rd[:nbytes]).cpu().numpy()), bits(want[:rows])), rows
        if spectra_rows:
            assert np.array_equal(bits(plan(bitfount.data_to_samples(rd[:nbytes])).cpu().numpy()), bits(want[:rows])), rows
            got = plan.spectra(Xd[: spectra_rows * K * N]).cpu().numpy()
            assert np.array_equal(bits(got), bits(want_spectra[:spectra_rows])), spectra_rows


def test_generic_across_the_chunk_loop(gpu, redio, oracle):
    """N = 4096, K = 17: 2100 transforms (17 MB of bytes) are 123 rows of two segments; a pass through the scratch takes 128 segments
    = 64 rows.  The first row, the rows either side of the seam and the last against the checker on their own windows."""
    N, K, ntr = 4096, 17, 2100
    rows = ntr // K
    chunk_rows = ((64 << 20) // (N * 8 * ref.SEG)) // 2
    assert rows == 123 and chunk_rows == 64
    raw = random_bytes(SEED + 1, 2 * ntr * N)
    plan = redio.PowerSpectrum(N, K)
    y = plan.u8(gpu.from_numpy(raw).cuda()).cpu().numpy()
    assert y.shape == (rows, N)
    for r in (0, chunk_rows - 1, chunk_rows, rows - 1):
        want = checker(oracle, raw[2 * r * K * N: 2 * (r + 1) * K * N], N, K, N, None)
        assert np.array_equal(bits(y[r]), bits(want[0])), r


CAPTURE = [(1024, 17, 512, 1), (1024, 17, 512, 2), (1000, 5, 1000, 0), (64, 33, 64, 0)]


@pytest.mark.parametrize("N,K,step,mode", CAPTURE)
def test_reserve_u8_then_capture_and_replay(gpu, redio, oracle, N, K, step, mode):
    w = window_of(oracle, N, True)
    W, H = ref.shape(N, K, step)
    raw = random_bytes(SEED + 3, 2 * (W + 3 * H))
    want = checker(oracle, raw, N, K, step, w)
    rd = gpu.from_numpy(raw).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K, step, w)
    plan.set_split(mode)
    plan.reserve_u8(raw.size)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan.u8(rd, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count  # reserved: the enqueue allocated nothing


def test_reserve_u8_covers_the_in_place_transform(gpu, redio, oracle):
    """N = 65536 un-windowed at step = N: the cf32 path never packs, so redio_pspec_reserve sizes no staging for the transform; the
    u8 call transforms in place through it, and reserve_u8 has to have sized it for the capture to go through"""
    N, K = 65536, 2
    raw = random_bytes(SEED + 8, 2 * K * N)
    want = checker(oracle, raw, N, K, N, None)
    rd = gpu.from_numpy(raw).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K)
    plan.reserve_u8(raw.size)
    g = redio.Graph()
    with g:
        plan.u8(rd, out=out)
    g.launch()
    gpu.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))


@pytest.mark.parametrize("N,K,mode", [(1024, 17, 2), (1000, 5, 0)])
def test_capture_needs_the_reserve(gpu, redio, oracle, N, K, mode):
    raw = random_bytes(SEED + 4, 2 * 2 * K * N)
    want = checker(oracle, raw, N, K, N, None)
    rd = gpu.from_numpy(raw).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K)
    plan.set_split(mode)
    g = redio.Graph()
    with pytest.raises(redio.RedioError) as e:
        with g:
            plan.u8(rd, out=out)
    assert e.value.code == ERR_NOT_RESERVED
    assert np.array_equal(bits(plan.u8(rd, out=out).cpu().numpy()), bits(want))  # the capture ended cleanly: the stream and the plan work on


def test_fused_row_mode_captures_without_a_reserve(gpu, redio, oracle):
    """(1024, 16) with a wave per row needs no scratch at all"""
    N, K = 1024, 16
    raw = random_bytes(SEED + 9, 2 * 2 * K * N)
    want = checker(oracle, raw, N, K, N, None)
    rd = gpu.from_numpy(raw).cuda()
    out = gpu.zeros(want.size, dtype=gpu.float32, device="cuda")
    plan = redio.PowerSpectrum(N, K)
    plan.set_split(1)
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan.u8(rd, out=out)
    g.launch()
    gpu.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(want.reshape(-1)))
    assert redio.lib().redio_malloc_count() == count


@pytest.mark.parametrize("N,K,step,windowed", [(1024, 17, 512, True), (64, 33, 64, False)])
def test_stream_gives_the_one_shot_bits(gpu, redio, oracle, N, K, step, windowed):
    """byte messages of any whole number of samples, a 1-sample one included: the concatenated rows are the one-shot u8 call's"""
    w = window_of(oracle, N, windowed)
    W, H = ref.shape(N, K, step)
    lens = [1, 7, W - 9, 1, H, W, W + 1, 3 * H + 5, 333, 2 * W + H - 1, 1, H - 1]
    raw = random_bytes(SEED + 5, 2 * sum(lens))
    rd = gpu.from_numpy(raw).cuda()
    plan = redio.PowerSpectrum(N, K, step, w)
    whole = plan.u8(rd)
    assert np.array_equal(bits(whole.cpu().numpy()), bits(checker(oracle, raw, N, K, step, w)))
    s = redio.Stream(plan, u8=True)
    for attempt in range(2):  # reset() starts over: the second pass repeats the first
        pos, outs, made = 0, [], 0
        for n in lens:
            expect = ref.nrows(pos + n, N, K, step) - made
            assert s.nout(n) == expect * N
            y = s(rd[2 * pos: 2 * (pos + n)])
            assert y.dtype == gpu.float32 and y.numel() == expect * N
            outs.append(y.clone())
            pos += n
            made += expect
            assert s.pending == pos - made * H
        assert gpu.equal(gpu.cat(outs), whole.reshape(-1)), (N, K, step, attempt)
        s.reset()
        assert s.pending == 0


@pytest.mark.parametrize("N,K", [(1024, 4), (512, 3)])
def test_misuse(gpu, redio, oracle, N, K):
    L = redio.lib()
    plan = redio.PowerSpectrum(N, K)
    n = 2 * K * N
    nbytes = 2 * n
    raw = random_bytes(SEED + 7, nbytes + 16)
    big = gpu.from_numpy(raw).cuda()
    out = gpu.full((2 * N + 2,), 7.0, dtype=gpu.float32, device="cuda")
    st = redio.current_stream()
    pb, po = big.data_ptr(), out.data_ptr()
    assert pb % 8 == 0 and po % 8 == 0
    fn = L.redio_pspec_enqueue_u8
    assert fn(plan._h, C.c_void_p(pb), nbytes - 1, C.c_void_p(po), st) == ERR_ARG          # odd nbytes
    assert fn(plan._h, C.c_void_p(pb + 1), nbytes, C.c_void_p(po), st) == ERR_ARG          # d_bytes at an odd address
    assert fn(plan._h, C.c_void_p(pb), nbytes, C.c_void_p(po + 2), st) == ERR_ARG          # d_out on a 2-byte boundary
    assert fn(plan._h, None, nbytes, C.c_void_p(po), st) == ERR_ARG
    assert fn(plan._h, C.c_void_p(pb), nbytes, None, st) == ERR_ARG
    assert fn(None, C.c_void_p(pb), nbytes, C.c_void_p(po), st) == ERR_ARG
    assert fn(plan._h, C.c_void_p(po + 4), nbytes, C.c_void_p(po), st) == ERR_ARG          # the bytes lie inside the output range
    assert fn(plan._h, C.c_void_p(pb), nbytes, C.c_void_p(pb + nbytes - 8), st) == ERR_ARG  # the output starts on the last four samples
    assert fn(plan._h, C.c_void_p(pb), 2 * (K * N - 1), C.c_void_p(po), st) == OK          # W - 1 samples: nothing to do
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all()) and np.array_equal(big.cpu().numpy(), raw)             # nothing was launched
    assert L.redio_pspec_reserve_u8(None, nbytes) == ERR_ARG
    assert fn(plan._h, C.c_void_p(pb + 2), nbytes, C.c_void_p(po), st) == OK               # a whole-sample boundary is enough
    gpu.cuda.synchronize()
    want = checker(oracle, raw[2: 2 + nbytes], N, K, N, None)
    assert np.array_equal(bits(out[: 2 * N].cpu().numpy()), bits(want.reshape(-1)))
    assert bool((out[2 * N:] == 7.0).all())


def test_stream_refuses_an_odd_address_before_it_launches(gpu, redio, oracle):
    """d_new of a u8 stream on an odd address: REDIO_ERR_ARG whatever the message's length, nothing staged, the stream where it was"""
    N, K = 64, 3
    W = K * N
    raw = random_bytes(SEED + 10, 2 * (3 * W) + 2)
    big = gpu.from_numpy(raw).cuda()
    plan = redio.PowerSpectrum(N, K)
    s = redio.Stream(plan, u8=True)
    first = s(big[: 2 * 10])  # ten samples carried
    assert first.numel() == 0 and s.pending == 10
    out = gpu.full((4 * N,), 7.0, dtype=gpu.float32, device="cuda")
    got = C.c_size_t(99)
    fn = redio.lib().redio_pspec_stream_enqueue
    for nsamp in (5, 2 * W):  # shorter than a window, and one that completes rows
        assert fn(s._h, C.c_void_p(big.data_ptr() + 21), nsamp, C.c_void_p(out.data_ptr()), C.byref(got), redio.current_stream()) == ERR_ARG
        assert got.value == 0 and s.pending == 10
    gpu.cuda.synchronize()
    assert bool((out == 7.0).all())
    y = s(big[20: 2 * (3 * W)])  # the stream goes on from its ten samples
    want = checker(oracle, raw[: 2 * (3 * W)], N, K, N, None)
    assert np.array_equal(bits(y.cpu().numpy()), bits(want.reshape(-1)))
