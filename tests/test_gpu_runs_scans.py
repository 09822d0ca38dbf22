"""The scans of the run-length / bit-field stage (runs.hip) past one wave and past one round, against tests/runs_ref.py: every run, every
byte, every f32 as bits.  scan_tiles_kernel needs more than 512 tiles (8 MiB) for its cross-wave sum and more than 8192 tiles (128 MiB)
for its carry; scan_u64_kernel needs more than 64 runs and more than 1024; rld_fill_kernel strides its grid from 16385 runs on."""
import ctypes as C

import numpy as np
import pytest

import runs_ref as ref

pytestmark = pytest.mark.gpu

TILE = 16384                      # RUN_TILE of runs.hip
ERR_ARG, ERR_UNSUPPORTED, ERR_ASSERT = -1, -3, -5
TIES = [(1 << 24) + 1, (1 << 24) + 3, (1 << 40) + (1 << 16), (1 << 40) + (1 << 16) + 1, (1 << 53) + 1, (1 << 54) + (1 << 30) + 1,
        1 << 63, (1 << 63) + (1 << 39), (1 << 63) + (1 << 39) + 1, (1 << 64) - 1]
NRUNS = [1, 2, 63, 64, 65, 128, 1023, 1024, 1025, 2049, 16384, 16385, 40000]


def f32bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def as_i64(gpu, a):
    """u64 bit patterns as the int64 device tensor the wrappers take"""
    return gpu.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


# ---- rle -------------------------------------------------------------------------------------------------------------------------------
def rle_seam_input(T, r):
    """T*16384 + r bytes, mostly constant.  A tile holds 0, 1, 2 or 7 changes, drawn at random, except that the four tiles around the first
    thread seam (8), every wave seam (512 k) and every round seam (8192 k) of scan_tiles_kernel hold 2, 7, 1, 0 -- four different partial
    sums, so that one taken a tile early or late, or dropped, moves a rank -- and that tiles 7, 511, T-1 and T/2 alternate on every byte
    (16384 changes each: the offsets pass 2^16 in front of the seams).  With r = 5 the ragged tile holds two more changes."""
    rng = np.random.default_rng(1000 * T + r)
    n = T * TILE + r
    per_tile = rng.choice([0, 1, 2, 7], T)
    for seam in [8] + list(range(512, T + 2, 512)):
        for d, c in zip((-2, -1, 0, 1), (2, 7, 1, 0)):
            if 0 <= seam + d < T:
                per_tile[seam + d] = c
    # up to 7 distinct offsets per tile, one per stratum of 2340 bytes, the strata in random order
    off = (np.arange(7) * 2340 + rng.integers(0, 2340, (T, 7)))[np.arange(T)[:, None], rng.random((T, 7)).argsort(1)]
    for seam in [8] + list(range(512, T + 1, 512)):          # changes on the first and the last byte of the tiles that meet at a seam
        if seam < T and per_tile[seam] >= 1:
            off[seam, 0] = 0
        if per_tile[seam - 1] >= 1:
            off[seam - 1, 0] = TILE - 1
    pos = (np.arange(T)[:, None] * TILE + off)[np.arange(7)[None, :] < per_tile[:, None]]
    alternating = sorted({t for t in (7, 511, T - 1, T // 2) if 0 <= t < T})
    pos = np.concatenate([pos] + [np.arange(t * TILE, (t + 1) * TILE) for t in alternating] + ([[n - 4, n - 2]] if r else []))
    pos = np.unique(pos[pos > 0])                           # the first byte ever is no change
    # run values over the whole byte range, neighbours different, with 255 -> 0 among them
    step = rng.integers(1, 256, len(pos) + 1)
    v = np.cumsum(step) % 256
    k = int(np.flatnonzero(v[:-1] == 255)[0])
    step[k + 1] = 1
    v = (np.cumsum(step) % 256).astype(np.uint8)
    assert v[k] == 255 and v[k + 1] == 0 and np.all(v[1:] != v[:-1])
    x = np.repeat(v, np.diff(np.concatenate(([0], pos, [n]))))
    assert len(x) == n
    return x


def check_feed(dev, d, x, st, what):
    v, c = dev.feed(d)
    wv, wc = ref.rle_np(x, st)
    assert v.numel() == len(wv), what
    assert np.array_equal(v.cpu().numpy(), wv), what
    assert np.array_equal(u64(c), wc), what
    return wv, wc


@pytest.mark.parametrize("r", [0, 5])
@pytest.mark.parametrize("T", [8, 9, 511, 512, 513, 1024, 8191, 8192, 8193])
def test_rle_tile_scan_seams(gpu, redio, T, r):
    x = rle_seam_input(T, r)
    d = gpu.from_numpy(x).cuda()
    wv, wc = check_feed(redio.kpn_dev.Rle(), d, x, ref.RleState(), (T, r))
    assert len(wv) > 1 << 14
    if T == 8193:
        # the same bytes in three calls: one byte, everything up to three bytes short of the round seam, the rest
        dev, st = redio.kpn_dev.Rle(), ref.RleState()
        cuts = [0, 1, 8192 * TILE - 3, len(x)]
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            check_feed(dev, d[lo:hi], x[lo:hi], st, (T, r, lo, hi))
    del d
    gpu.cuda.empty_cache()                                   # Rle.feed sizes its outputs for the worst case, 9 bytes per input byte


def test_rle_refuses_a_result_that_does_not_fit_without_consuming(gpu, redio):
    """A call whose completed runs exceed cap returns REDIO_ERR_ARG and consumes nothing: the same call with room gives what the reference
    gives from the state BEFORE the refused call, and so does the call after it."""
    rng = np.random.default_rng(12)
    x = np.repeat(rng.integers(0, 256, 30000), rng.integers(1, 9, 30000)).astype(np.uint8)
    a, b = 3 * TILE + 11, 5 * TILE + 2                       # three calls: [0, a), [a, b), [b, len)
    assert len(x) > b + 100
    d = gpu.from_numpy(x).cuda()
    L = redio.lib()
    h = C.c_void_p()
    assert L.redio_rle_create(C.byref(h)) == 0
    st = ref.RleState()
    vals = gpu.full((len(x),), 0xEE, dtype=gpu.uint8, device="cuda")
    cnts = gpu.full((len(x),), -2, dtype=gpu.int64, device="cuda")
    nr = C.c_size_t(0)

    def feed(lo, hi, cap):
        return L.redio_rle_feed(h, C.c_void_p(d.data_ptr() + lo), hi - lo, C.c_void_p(vals.data_ptr()), C.c_void_p(cnts.data_ptr()), cap,
                                C.byref(nr), None)

    def same(want):
        k = len(want[0])
        return nr.value == k and np.array_equal(vals[:k].cpu().numpy(), want[0]) and np.array_equal(u64(cnts[:k]), want[1])

    assert feed(0, a, len(x)) == 0 and same(ref.rle_np(x[:a], st))
    before = st.copy()
    want = ref.rle_np(x[a:b], st)
    assert len(want[0]) > 1000
    vals.fill_(0xEE); cnts.fill_(-2)
    for cap in (len(want[0]) - 1, 0):
        assert feed(a, b, cap) == ERR_ARG
    gpu.cuda.synchronize()
    assert bool((vals == 0xEE).all()) and bool((cnts == -2).all())            # and nothing was written
    assert feed(a, b, len(want[0])) == 0 and same(want)                         # exactly enough room
    assert same(ref.rle_np(x[a:b], before))                                     # = the reference from the state before the refusal
    assert feed(b, len(x), len(x)) == 0 and same(ref.rle_np(x[b:], st))
    L.redio_rle_destroy(h)


# ---- rld / dld -------------------------------------------------------------------------------------------------------------------------
def rld_counts(nruns, rng):
    """counts around the 256-thread block of the fill, zeros at the first and the last run and at the first lane of a wave (64), of a
    round (1024) and of a second pass of the grid (16384), a non-zero count in the lane a round's carry is taken from (1023), one run of 2^20"""
    if nruns <= 2:
        return np.array([0, 1 << 20][-nruns:], np.uint64)
    c = rng.choice([0, 1, 2, 255, 256, 257, 1000], nruns).astype(np.uint64)
    zero = [k for k in (0, 63, 64, 1024, 16384, nruns - 1) if k < nruns]
    full = [k for k in (62, 1023, 2047, 16383) if k < nruns - 1]
    c[full] = 257
    c[zero] = 0
    big = next(k for k in range(nruns // 2, nruns) if k not in zero + full)
    c[big] = 1 << 20
    return c


@pytest.mark.parametrize("nruns", NRUNS)
def test_rld_run_count_seams(gpu, redio, nruns):
    rng = np.random.default_rng(nruns)
    counts = rld_counts(nruns, rng)
    vals = rng.integers(0, 256, nruns).astype(np.uint8)
    want = ref.rld_ref(vals, counts)
    assert len(want) >= 1 << 20
    got = redio.kpn_dev.rld(gpu.from_numpy(vals).cuda(), as_i64(gpu, counts))
    assert got.numel() == len(want)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize("nruns", [1, 65, 1025, 16385])
def test_rld_all_zero_counts_give_nothing(gpu, redio, nruns):
    vals = gpu.zeros(nruns, dtype=gpu.uint8, device="cuda")
    got = redio.kpn_dev.rld(vals, gpu.zeros(nruns, dtype=gpu.int64, device="cuda"))    # the wrapper raises unless rc == 0
    assert got.numel() == 0


def test_rld_refuses_an_output_one_byte_short_and_reports_the_total(gpu, redio):
    rng = np.random.default_rng(77)
    nruns = 1025
    counts = rld_counts(nruns, rng)
    total = int(counts.sum())
    vals = gpu.from_numpy(rng.integers(0, 256, nruns).astype(np.uint8)).cuda()
    dc = as_i64(gpu, counts)
    out = gpu.full((total + 64,), 0xA5, dtype=gpu.uint8, device="cuda")
    scratch = gpu.empty(nruns + 1, dtype=gpu.int64, device="cuda")
    no = C.c_size_t(0)
    L = redio.lib()

    def call(cap):
        return L.redio_rld(C.c_void_p(vals.data_ptr()), C.c_void_p(dc.data_ptr()), nruns, C.c_void_p(out.data_ptr()), cap,
                           C.c_void_p(scratch.data_ptr()), C.byref(no), None)

    assert call(total - 1) == ERR_ARG and no.value == total
    gpu.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert call(total) == 0 and no.value == total
    gpu.cuda.synchronize()
    assert np.array_equal(out[:total].cpu().numpy(), ref.rld_ref(vals.cpu().numpy(), counts))
    assert bool((out[total:] == 0xA5).all())


def dld_durations(nruns, rate, rng):
    """random durations below 4 ms with the special ones mixed in: NaN, negative, both zeros, the smallest subnormal, the f32 just below
    k / rate, and dle's own k / rate for k = 1 .. 2000 -- the round trip of the shipped graph"""
    f = np.float32
    dur = (rng.random(nruns) * 0.004).astype(np.float32)
    assert dur.max() < f(0.004)
    special = np.concatenate((
        np.array([np.nan, -1.0, -0.0, 0.0], np.float32), np.array([1], np.uint32).view(np.float32),
        np.array([np.nextafter(f(k) / f(rate), f(0)) for k in (1, 2, 3, 64, 255, 256, 257, 1000, 1023, 1024)], np.float32),
        ref.dle_ref(np.arange(1, 2001, dtype=np.uint64), int(rate))))
    m = min(len(special), max(1, nruns // 2) if nruns < 16384 else nruns)
    dur[rng.permutation(nruns)[:m]] = special[: m] if m == len(special) else rng.permutation(special)[:m]
    return dur


@pytest.mark.parametrize("rate", [256000.0, 48000.0])
@pytest.mark.parametrize("nruns", NRUNS)
def test_dld_durations_to_runs(gpu, redio, nruns, rate):
    rng = np.random.default_rng(nruns + int(rate))
    dur = dld_durations(nruns, rate, rng)
    vals = rng.integers(0, 256, nruns).astype(np.uint8)
    counts = ref.dld_counts_ref(dur, rate)
    want = ref.rld_ref(vals, counts)
    got = redio.kpn_dev.dld(gpu.from_numpy(vals).cuda(), gpu.from_numpy(dur).cuda(), rate, len(want))
    assert got.numel() == len(want)
    assert np.array_equal(got.cpu().numpy(), want)


def test_dld_round_trips_every_count_that_dle_makes(gpu, redio):
    # all of k / rate for k = 1 .. 2000 in ONE call (dld_durations draws from them where nruns is small), with device-made durations
    for rate in (256000, 48000):
        k = np.arange(1, 2001, dtype=np.uint64)
        vals = (k % 256).astype(np.uint8)
        sec = redio.kpn_dev.dle(as_i64(gpu, k), rate)
        assert np.array_equal(f32bits(sec.cpu().numpy()), f32bits(ref.dle_ref(k, rate)))
        counts = ref.dld_counts_ref(ref.dle_ref(k, rate), float(rate))
        got = redio.kpn_dev.dld(gpu.from_numpy(vals).cuda(), sec, float(rate), int(counts.sum()))
        assert np.array_equal(got.cpu().numpy(), ref.rld_ref(vals, counts))


@pytest.mark.parametrize("dur", [np.inf, 1e30])
def test_dld_refuses_a_saturated_count_and_writes_nothing(gpu, redio, dur):
    cap = 16
    vals = gpu.tensor([7], dtype=gpu.uint8, device="cuda")
    sec = gpu.tensor([dur], dtype=gpu.float32, device="cuda")
    out = gpu.full((cap + 64,), 0xA5, dtype=gpu.uint8, device="cuda")
    scratch = gpu.empty(3, dtype=gpu.int64, device="cuda")
    no = C.c_size_t(0)
    rc = redio.lib().redio_dld(C.c_void_p(vals.data_ptr()), C.c_void_p(sec.data_ptr()), 1, 256000.0, C.c_void_p(out.data_ptr()), cap,
                               C.c_void_p(scratch.data_ptr()), C.byref(no), None)
    assert rc == ERR_ARG
    assert no.value == int(ref.dld_counts_ref(np.float32(dur), 256000.0)[0]) == (1 << 64) - 1
    gpu.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert redio.kpn_dev.dld(vals, gpu.tensor([3.0 / 256000.0], dtype=gpu.float32, device="cuda"), 256000.0, cap).cpu().tolist() == [7] * 3


# ---- dle -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s_rate", [256000, 1, 16777217, 0])
def test_dle_converts_u64_counts_with_one_rounding(gpu, redio, s_rate):
    rng = np.random.default_rng(4)
    cts = np.concatenate((np.array(TIES + [0], np.uint64), rng.integers(0, 1 << 64, 10000, dtype=np.uint64)))
    got = redio.kpn_dev.dle(as_i64(gpu, cts), s_rate).cpu().numpy()
    want = ref.dle_ref(cts, s_rate)
    bad = np.flatnonzero(f32bits(got) != f32bits(want))
    assert bad.size == 0, [(int(cts[i]), hex(f32bits(got)[i]), hex(f32bits(want)[i])) for i in bad[:8]]


# ---- binconv ---------------------------------------------------------------------------------------------------------------------------
NMSG = [1, 51, 52, 255, 257, 1000]            # 51 * 5 = 255 and 52 * 5 = 260 threads; 255 and 257 straddle a block with one field


def check_binconv(gpu, redio, digits, widths):
    got = redio.kpn_dev.binconv(gpu.from_numpy(digits).cuda(), widths)
    assert tuple(got.shape) == (digits.shape[0], len(widths))
    want = ref.binconv_ref(digits, widths)
    assert np.array_equal(u64(got), want), widths


@pytest.mark.parametrize("nmsg", NMSG)
def test_binconv_every_single_width(gpu, redio, nmsg):
    rng = np.random.default_rng(nmsg)
    digits = rng.integers(0, 2, (nmsg, 64)).astype(np.uint8)
    digits[0] = 1                                             # 2^w - 1: every term of the sum, 1 << 63 among them
    for w in range(65):
        check_binconv(gpu, redio, digits, [w])


@pytest.mark.parametrize("nmsg", NMSG)
@pytest.mark.parametrize("widths,extra", [([64], 0), ([63, 1], 0), ([0, 64, 0], 0), ([1] * 64, 0), ([32, 32], 0), ([4, 8, 4, 12, 8], 0),
                                          ([4, 8, 4, 12, 8], 3)])
def test_binconv_width_lists(gpu, redio, widths, extra, nmsg):
    rng = np.random.default_rng(nmsg + len(widths))
    digits = rng.integers(0, 2, (nmsg, sum(widths) + extra)).astype(np.uint8)
    digits[0] = 1
    check_binconv(gpu, redio, digits, widths)


def test_binconv_multiplies_digits_beyond_one(gpu, redio):
    # b2d multiplies the digit (kpn.rs:112); at widths <= 48 a sum of 255 * 2^k stays below 2^56
    rng = np.random.default_rng(6)
    digits = rng.integers(0, 256, (257, 64)).astype(np.uint8)
    digits[0], digits[1] = 255, 2
    for widths in ([48, 3, 13], [1] * 64, [8, 8, 8, 8], [48]):
        check_binconv(gpu, redio, digits, widths)


def test_binconv_refusals_leave_the_library_working(gpu, redio):
    digits = np.ones((3, 64), np.uint8)
    d = gpu.from_numpy(digits).cuda()
    for widths, code in (([1] * 65, ERR_UNSUPPORTED), ([65], ERR_UNSUPPORTED), ([60, 5], ERR_ASSERT), ([64, 1], ERR_ASSERT)):
        with pytest.raises(redio.RedioError) as e:
            redio.kpn_dev.binconv(d, widths)
        assert e.value.code == code, widths
    check_binconv(gpu, redio, digits, [60, 4])                # a sum equal to nbits is fine
    check_binconv(gpu, redio, digits, [64])


# ---- the stage end to end --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(30))
def test_round_trip_of_random_cut_streams(gpu, redio, seed):
    """rld(rle(x)), concatenated over the calls, is x without its open last run; dld(dle(counts)) is rld over the reference's counts"""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 300001)) if seed else 1
    scale = int(rng.choice([1, 2, 30, 3000]))
    nv = int(rng.choice([2, 3, 256]))
    m = 2 * n // scale + 2
    x = np.repeat(rng.integers(0, nv, m), rng.integers(1, scale + 1, m)).astype(np.uint8)[:n]
    n = len(x)
    off = int(rng.integers(0, 9))
    buf = gpu.empty(n + off, dtype=gpu.uint8, device="cuda")
    buf[off:] = gpu.from_numpy(x)
    cuts = sorted(set(rng.integers(1, n + 1, int(rng.integers(1, 5))).tolist()) | {0, n})
    rate = int(rng.choice([256000, 48000]))
    dev, st = redio.kpn_dev.Rle(), ref.RleState()
    back, back_d = [], []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v, c = dev.feed(buf[off + lo:off + hi])
        wv, wc = ref.rle_np(x[lo:hi], st)
        assert np.array_equal(v.cpu().numpy(), wv) and np.array_equal(u64(c), wc), (lo, hi)
        back.append(redio.kpn_dev.rld(v, c).cpu().numpy())
        sec = redio.kpn_dev.dle(c, rate)
        want_sec = ref.dle_ref(wc, rate) if len(wc) else np.empty(0, np.float32)
        assert np.array_equal(f32bits(sec.cpu().numpy()), f32bits(want_sec))
        want_d = ref.rld_ref(wv, ref.dld_counts_ref(want_sec, float(rate))) if len(wc) else np.empty(0, np.uint8)
        assert np.array_equal(redio.kpn_dev.dld(v, sec, float(rate), len(want_d)).cpu().numpy(), want_d), (lo, hi)
    changes = np.flatnonzero(x[1:] != x[:-1])
    closed = int(changes[-1]) + 1 if len(changes) else 0      # the open run starts at the last change
    assert np.array_equal(np.concatenate(back), x[:closed])
