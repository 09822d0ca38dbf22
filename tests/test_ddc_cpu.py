"""The tuner (redio_ddc_*) without a GPU: the oscillator table generator against its rule restated in Python, the kernels' loader and
lane programs emulated thread by thread on the CPU (tests/emu_ddc, the device's own headers) against the oracle's mul_vecs + fir, and
the first_index the carried-history layer hands to the head and the body of a call against a model of the stream.  The last tap count
the chunked route takes at each decimation is pinned, the restatement (tests/ddc_ref.py) is compared with the device headers' own
numbers, and the loader and lane program run at that limit, where the table indices reach farthest."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ddc_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDDDC0


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_ddc"), "-s"])
    L = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_ddc.so"))
    vp, i, l, u64 = C.c_void_p, C.c_int, C.c_long, C.c_uint64
    L.emu_ddc_tile.restype = i
    L.emu_ddc_tile.argtypes = [i, l, i, i, vp, l, u64, vp, C.c_uint, vp, l, i, vp, vp, C.POINTER(i), C.POINTER(i), C.POINTER(i)]
    L.emu_ddc_route.restype = i
    L.emu_ddc_route.argtypes = [l, l]
    L.emu_ddc_chunked_tile_in.restype = L.emu_ddc_chunked_lds_elems.restype = l
    L.emu_ddc_chunked_tile_in.argtypes = L.emu_ddc_chunked_lds_elems.argtypes = [l, l]
    L.emu_ddc_chunked_chw.restype = i
    L.emu_ddc_chunked_chw.argtypes = [l]
    L.emu_ddc_stream_step.restype = None
    L.emu_ddc_stream_step.argtypes = [vp, C.c_size_t, C.c_size_t, C.c_size_t, vp]
    return L


@pytest.mark.parametrize("num,den", [(1, 1), (1, 2), (1, 4), (-1, 4), (3, 4), (1, 24), (-5, 24), (7, 1000), (1, 4099), (1, 65536), (-1, 65536), (6, 24)])
def test_osc_table_is_its_rule_bit_for_bit(redio, num, den):
    got, want = redio.dsputils.osc_table(num, den), ref.osc_table_ref(num, den)
    assert len(got) == len(want) == redio.dsputils.osc_table(num, den).size
    assert np.array_equal(bits(got), bits(want))
    if (num, den) == (6, 24):
        assert np.array_equal(got, np.array([1, 1j, -1, -1j], np.complex64))  # period 4, every entry exact


def test_osc_table_period_and_refusals(redio):
    period = C.c_size_t(0)
    assert redio.lib().redio_osc_table(-10, 24, None, C.byref(period)) == 0 and period.value == 12  # NULL out: the period alone
    assert redio.lib().redio_osc_table(1, 0, None, C.byref(period)) == -1
    assert redio.lib().redio_osc_table(1, 65537, None, C.byref(period)) == -1  # period above REDIO_DDC_MAX_PERIOD
    assert redio.lib().redio_osc_table(2, 131072, None, C.byref(period)) == 0 and period.value == 65536
    with pytest.raises(redio.RedioError):
        redio.dsputils.osc_table(1, 0)


def table_ext(emu, w):
    """the device table's layout (ddc_api.hip): the period, then DDC_TABLE_EXT more entries of it; a fence of -1 behind"""
    n = len(w) + emu.emu_ddc_table_ext()
    t = np.full(n + 4096, -1, np.complex64)
    t[:n] = w[np.arange(n) % len(w)]
    return t, n


def run_tile(emu, K, D, u8, fused, x, n_in, first, tab, L, taps, tile, vec, lanes=True):
    """lanes=False: the loader alone, no outputs"""
    image = np.empty(20000, np.complex64)
    y = np.empty(2048, np.complex64)
    ti, to, bad = C.c_int(0), C.c_int(0), C.c_int(0)
    route = emu.emu_ddc_tile(K, D, int(u8), int(fused), x.ctypes.data, n_in, first, tab.ctypes.data, L, taps.ctypes.data, tile, int(vec),
                             image.ctypes.data, y.ctypes.data if lanes else None, C.byref(ti), C.byref(to), C.byref(bad))
    assert bad.value == 0, "an image write outside the LDS allocation"
    return route, image[: ti.value], y[: to.value] if lanes else None, ti.value, to.value


# (taps, decimation): every tile geometry of the three routes
SHAPES = [(127, 5), (63, 1), (31, 2), (17, 3), (255, 10), (5, 9)]
PERIODS = [1, 3, 24, 4099, 65536]


@pytest.mark.parametrize("K,D", SHAPES)
def test_loader_and_lane_program_emulated(emu, oracle, K, D):
    """tile 0, a tile whose (first + in0) mod L lies within one tile of L, and the last partial tile; the 16-byte and scalar cf32 paths
    and the u8 paths; every table index inside the allocation and equal to (first + n) mod L; the image and the outputs equal ddc_ref's"""
    rng = np.random.default_rng(SEED + 131 * K + D)
    route = emu.emu_ddc_route(K, D)
    assert route == ref.route(K, D)
    TO = ref.tile_out(K, D)
    n_out = 2 * TO + 37
    n = (n_out - 1) * D + K + (D - 1)
    taps = np.zeros((K + 15) // 16 * 16, np.float32)
    taps[:K] = oracle.synth_f32(3, K, K)
    xc = oracle.synth_iq(SEED, K, n)
    raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    ones_c, ones_b = np.ones(n, np.complex64), np.tile(np.array([254, 127], np.uint8), n)  # i2f(254) = 1, i2f(127) = 0
    case = 0
    for L in PERIODS:
        w = (oracle.synth_iq(7, L, L) if L != 24 else ref.osc_table_ref(-5, 24)).astype(np.complex64)
        tab, nalloc = table_ext(emu, w)
        probe = np.full(len(tab), -1, np.complex64)
        probe[:nalloc] = np.arange(nalloc, dtype=np.float32)  # entry e reads back as e through a sample of (1, 0)
        in0_1 = TO * D  # the second tile's first sample
        for first in [0, L - 1, 2 ** 32 + 5, 2 ** 64 - 1 - n, (L - 5 - in0_1) % L]:
            for u8 in (False, True):
                fused = bool(case & 1)
                case += 1
                want_m = ref.mixed(oracle.data_to_samples(raw) if u8 else xc, w, first)
                want_y = oracle.fir(want_m, taps[:K], D, fused)
                assert len(want_y) == n_out
                for vec in (True, False):
                    for tile in (0, 1, 2):
                        x = raw if u8 else xc
                        r, image, y, tile_in, tile_out = run_tile(emu, K, D, u8, fused, x, n, first, tab, L, taps, tile, vec)
                        assert r == route and tile_out == TO
                        o0, in0 = tile * TO, tile * TO * D
                        valid = min(TO, n_out - o0)
                        assert valid > 0 and (tile < 2 or valid == 37)
                        assert np.array_equal(bits(y[:valid]), bits(want_y[o0: o0 + valid])), (L, first, u8, vec, tile)
                        if route == 3:
                            continue
                        have = min(tile_in, n - in0)
                        assert np.array_equal(bits(image[:have]), bits(want_m[in0: in0 + have])), (L, first, u8, vec, tile)
                        assert not image[have:].view(np.float32).any()  # beyond n_in: zeros, written without a table read
                        # the table indices: the same loader on samples of (1, 0) and a table whose entry e holds e
                        _, pimg, _, _, _ = run_tile(emu, K, D, u8, fused, ones_b if u8 else ones_c, n, first, probe, L, taps, tile, vec)
                        e = pimg[:have].real.astype(np.int64)
                        assert (pimg[:have].imag == 0).all() and (e >= 0).all() and (e < nalloc).all()
                        wantidx = np.array([(first + in0 + i) % L for i in range(have)], np.int64)
                        assert np.array_equal(e % L, wantidx) and e[0] < L and np.array_equal(e - e[0], np.arange(have))


# decimation: (the last tap count the chunked route takes, the samples its workgroup stages there) -- 150 KiB of LDS; one tap more
# goes to the direct route
LAST_CHUNKED = {1: (15008, 17055), 2: (15008, 17054), 3: (14640, 17709), 4: (13968, 18060), 5: (13152, 18267), 8: (13968, 18056),
                10: (13168, 18278)}


def test_last_chunked_tap_counts_are_pinned():
    """the table, recomputed from the restatement, and the design argument of ddc_core.h at each row: a lane reads table entry
    base + n for n < tile_in + 2, inside the 20480 entries behind the period"""
    assert set(LAST_CHUNKED) == set(ref.CHUNKED_R)
    for D, (K, tile_in) in LAST_CHUNKED.items():
        assert ref.last_chunked(D) == K and ref.tile_in(K, D) == tile_in
        assert ref.route(K, D) == 2 and ref.route(K + 1, D) == 3
        assert ref.lds_elems(K, D) * 8 <= ref.CHUNKED_LDS_MAX < ref.lds_elems(K + 1, D) * 8
        assert ref.tile_out(K, D) == 256 * ref.CHUNKED_R[D] and ref.tile_out(K + 1, D) == 256
        assert tile_in + 2 <= 20480 == ref.TABLE_EXT
    assert ref.route(2 ** 20, 7) == ref.route(300, 9) == 3  # no chunked form at these decimations
    assert [ref.route(K, D) for K, D in [(127, 5), (63, 1), (127, 2), (64, 1)]] == [1, 1, 2, 2]


def test_restatement_agrees_with_the_device_headers(emu):
    """ddc_route, ddc_chunked_tile_in, ddc_chunked_lds_elems and ddc_chunked_chw as the headers compute them, at every pinned tap count and
    its two neighbours, at the chunk sizes' neighbours and at small counts, every decimation of the chunked route and two without one"""
    assert emu.emu_ddc_table_ext() == ref.TABLE_EXT
    for D in list(ref.CHUNKED_R) + [7, 9]:
        near = LAST_CHUNKED.get(D, (15008,))[0]
        for K in sorted({1, 2, 15, 16, 17, 63, 64, 127, 128, 300, 4097, near - 1, near, near + 1, 20000, 2 ** 20, 2 ** 20 + 1, 2 ** 24}):
            assert emu.emu_ddc_route(K, D) == ref.route(K, D), (K, D)
            if D in ref.CHUNKED_R:
                assert emu.emu_ddc_chunked_tile_in(K, D) == ref.tile_in(K, D), (K, D)
                assert emu.emu_ddc_chunked_lds_elems(K, D) == ref.lds_elems(K, D), (K, D)
                assert emu.emu_ddc_chunked_chw(D) == ref.chw(D)
                if ref.route(K, D) == 2:
                    assert ref.tile_in(K, D) + 2 <= emu.emu_ddc_table_ext()  # what launch_chunked refuses otherwise
            else:
                assert emu.emu_ddc_chunked_lds_elems(K, D) == 0


@pytest.mark.parametrize("K,D", [(15008, 1), (13168, 10)])
def test_loader_and_lane_program_emulated_at_the_lds_limit(emu, oracle, K, D):
    """the longest tiles the chunked route stages (150 KiB): one whole tile and the partial one behind it, periods 1 and 65536, the
    first workgroup's table base odd (L - 1: 8-byte table loads), even, and within one tile of L; cf32 and u8, wide and scalar sample
    loads.  Every table index is inside the allocation; the image and the outputs equal ddc_ref's, so no lane program read left the
    LDS allocation (the emulator's image has exactly ddc_chunked_lds_elems elements between fences of NaN)."""
    rng = np.random.default_rng(SEED + 131 * K + D)
    assert emu.emu_ddc_route(K, D) == ref.route(K, D) == 2 and emu.emu_ddc_route(K + 1, D) == ref.route(K + 1, D) == 3
    TO = ref.tile_out(K, D)
    n_out = TO + 37
    n = (n_out - 1) * D + K + (D - 1)
    taps = oracle.synth_f32(3, K, K)
    assert len(taps) % 16 == 0  # the device's taps need no padding here
    xc = oracle.synth_iq(SEED, K, n)
    raw = rng.integers(0, 256, 2 * n, dtype=np.uint8)
    ones_c, ones_b = np.ones(n, np.complex64), np.tile(np.array([254, 127], np.uint8), n)  # i2f(254) = 1, i2f(127) = 0
    case = 0
    for L in (1, 65536):
        w = oracle.synth_iq(7, L, L).astype(np.complex64)
        tab, nalloc = table_ext(emu, w)
        probe = np.full(len(tab), -1, np.complex64)
        probe[:nalloc] = np.arange(nalloc, dtype=np.float32)  # entry e reads back as e through a sample of (1, 0)
        firsts = [0] if L == 1 else [L - 1, 2 ** 32 + 6, (L - 5 - TO * D) % L]
        bases = set()
        for first in firsts:
            for u8 in (False, True):
                fused = bool(case & 1)
                case += 1
                want_m = ref.mixed(oracle.data_to_samples(raw) if u8 else xc, w, first)
                want_y = oracle.fir(want_m, taps, D, fused)
                assert len(want_y) == n_out
                for vec in (True, False):
                    for tile in (0, 1):
                        x = raw if u8 else xc
                        r, image, y, tile_in, tile_out = run_tile(emu, K, D, u8, fused, x, n, first, tab, L, taps, tile, vec)
                        assert r == 2 and tile_out == TO and tile_in == ref.tile_in(K, D) == LAST_CHUNKED[D][1]
                        o0, in0 = tile * TO, tile * TO * D
                        valid = min(TO, n_out - o0)
                        assert valid == (TO if tile == 0 else 37)
                        assert np.array_equal(bits(y[:valid]), bits(want_y[o0: o0 + valid])), (L, first, u8, vec, tile)
                        have = min(tile_in, n - in0)
                        assert np.array_equal(bits(image[:have]), bits(want_m[in0: in0 + have])), (L, first, u8, vec, tile)
                        assert not image[have:].view(np.float32).any()  # beyond n_in: zeros, written without a table read
                        _, pimg, _, _, _ = run_tile(emu, K, D, u8, fused, ones_b if u8 else ones_c, n, first, probe, L, taps, tile, vec, lanes=False)
                        e = pimg[:have].real.astype(np.int64)
                        assert (pimg[:have].imag == 0).all() and (e >= 0).all() and (e < nalloc).all()
                        assert e[0] == (first + in0) % L and np.array_equal(e - e[0], np.arange(have))
                        bases.add(int(e[0]) & 1)
                        if tile == 0:
                            assert have == tile_in and e[-1] == e[0] + tile_in - 1  # the whole tile is there: the farthest index a lane forms
        assert bases == ({0} if L == 1 else {0, 1})


@pytest.mark.parametrize("W,H", [(127, 5), (31, 2), (5, 9), (1, 1), (4, 4), (3, 7)])
def test_stream_split_hands_out_the_phase(emu, W, H):
    """random cuts: the head and the body of every call start at the unit the stream has reached -- first_index = unit * H"""
    rng = np.random.default_rng(SEED + W)
    for trial in range(40):
        state = np.zeros(4, np.uint64)
        out = np.zeros(4, np.uint64)
        total = units = 0
        for _ in range(30):
            n = int(rng.choice([0, 1, 2, W - 1, W, W + 1, int(rng.integers(0, 4 * W + 3 * H)), int(rng.integers(0, 40 * H))]))
            emu.emu_ddc_stream_step(state.ctypes.data, W, H, n, out.ctypes.data)
            nh, head_first, nb, body_first = (int(v) for v in out)
            if nh:
                assert head_first == units * H
            if nb:
                assert body_first == (units + nh) * H
            total += n
            units += nh + nb
            assert int(state[2]) == total and int(state[3]) == units  # redio_ddc_stream_index after the call
            assert units == (0 if total < W else (total - W) // H + 1)
