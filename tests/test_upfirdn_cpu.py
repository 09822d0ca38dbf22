"""The rational resampler (redio_upfirdn_*) without a GPU: the phase table against brute force over the taps, the output count against the
oracle's FIR on the zero-stuffed stream, the per-phase reference (tests/upfirdn_ref.py) against that zero-stuffed form, the stream's
segmentation in periods against a model, and the kernels emulated thread by thread on the CPU (tests/emu_upfirdn, the device's own
headers) against the contract written out -- at the shapes of the GPU tests and at long filters, where the tile is 52 to 150 KiB.  The
regimes of route 1's tile geometry over the tap count are pinned, and the restatement is compared with the device headers' own numbers."""
import os
import subprocess

import numpy as np
import pytest

import upfirdn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDF1D0

# (U, D, K): the fifteen shapes of the issue's CPU check, 1/5/127 to 160/147/481 -- every GPU shape of tests/test_gpu_upfirdn.py
SHAPES = [(1, 5, 127), (2, 1, 63), (3, 2, 64), (2, 3, 31), (4, 5, 100), (5, 4, 127), (16, 1, 255), (3, 8, 17), (7, 10, 40), (6, 4, 50),
          (5, 1, 3), (160, 147, 481), (3, 16, 33), (17, 1, 40), (2, 7, 9)]
ROUTE1 = SHAPES[:11]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("U,D,K", SHAPES)
def test_phase_table_against_brute_force(U, D, K):
    Up, Dp = ref.periods(U, D)
    table = ref.phases(K, U, D)
    assert len(table) == Up and Up * D == Dp * U
    reach = 1
    for q in (0, 1, 7):
        for r, (j0, s, k) in enumerate(table):
            i = r + Up * q
            js = [j for j in range(K) if (i * D + j) % U == 0]  # the taps that meet a sample of x
            assert len(js) == k
            if js:
                assert js[0] == j0 and js == list(range(j0, K, U))
                assert [(i * D + j) // U for j in js] == list(range(q * Dp + s, q * Dp + s + k))
            if q == 0:
                reach = max(reach, s + k)
    assert ref.window(K, U, D) == reach


@pytest.mark.parametrize("U,D,K", SHAPES)
def test_nout_is_the_count_of_the_fir_on_the_zero_stuffed_stream(oracle, U, D, K):
    taps = oracle.synth_f32(1, 0, K)
    for n in [0, 1, K // U, K // U + 1, -(-K // U), -(-K // U) + 1, 100, 1001]:
        got = oracle.fir(np.zeros(n * U, np.float32), taps, D)
        assert ref.nout(n, K, U, D) == len(got), n


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("U,D,K", SHAPES)
def test_per_phase_reference_equals_the_zero_stuffed_form(oracle, U, D, K, cplx, fused):
    taps = oracle.synth_f32(3, K, K)
    for n in [0, 1, 17, 256, 1000, 4099]:
        x = oracle.synth_iq(SEED, U + D, n) if cplx else oracle.synth_f32(SEED, U + D, n)
        got, want = ref.upfirdn(x, taps, U, D, fused), ref.upfirdn_zero_stuffed(x, taps, U, D, fused)
        assert got.dtype == want.dtype and got.shape == want.shape
        assert np.array_equal(bits(got), bits(want)), n


def test_route_and_tile_geometry():
    for U, D, K in ROUTE1:
        assert ref.route(K, U, D) == 1 and ref.periods_per_lane(K, U, D) in (1, 2, 4)
        assert ref.lds_elems(ref.periods_per_lane(K, U, D), K, U, D) * 8 <= ref.LDS_MAX
    for U, D, K in SHAPES[11:]:
        assert ref.route(K, U, D) == 2 and ref.tile_out(K, U, D) == 256
    assert ref.route(1 << 21, 2, 1) == 2      # above the tiled kernel's tap count
    assert ref.route(40000 * 2, 2, 1) == 2    # a window that no tile holds
    assert ref.periods_per_lane(63, 2, 1) == 4 and ref.periods_per_lane(127, 4, 5) == 2 and ref.periods_per_lane(255, 16, 1) == 1


# (U, D): [(the first K of a regime, R, pass of upfirdn_r, route)], K up to 2^20.  Pass 2 is the tiles of 52 to 150 KiB; R 0 is route 2
REGIMES = {
    (2, 1): [(1, 4, 1, 1), (5326, 2, 1, 1), (6486, 1, 1, 1), (11776, 4, 2, 1), (25396, 1, 2, 1), (36864, 0, 0, 2)],
    (3, 2): [(1, 4, 1, 1), (3414, 2, 1, 1), (9216, 1, 1, 1), (10242, 4, 2, 1), (36864, 2, 2, 1), (39324, 0, 0, 2)],
    (2, 3): [(1, 4, 1, 1), (2366, 2, 1, 1), (6586, 1, 1, 1), (10754, 4, 2, 1), (25524, 2, 2, 1), (28090, 1, 2, 1), (35842, 0, 0, 2)],
    (4, 5): [(1, 2, 1, 1), (6522, 1, 1, 1), (17410, 4, 2, 1), (37062, 2, 2, 1), (52134, 1, 2, 1), (67586, 0, 0, 2)],
    (3, 8): [(1, 2, 1, 1), (2175, 1, 1, 1), (9564, 2, 2, 1), (37593, 1, 2, 1), (43014, 0, 0, 2)],
    (7, 10): [(1, 1, 1, 1), (13038, 2, 2, 1), (68275, 1, 2, 1), (92866, 0, 0, 2)],
    (16, 1): [(1, 1, 1, 1), (36850, 2, 2, 1), (109218, 1, 2, 1), (237554, 0, 0, 2)],
}
# (U, D, K): cf32 bytes of the tile, window
TILES = {(2, 1, 11776): (85536, 5889), (2, 1, 25396): (107744, 12699), (3, 2, 10242): (73760, 3416), (3, 2, 36864): (145440, 12290),
         (4, 5, 17410): (112352, 4357), (3, 8, 37593): (137344, 12537), (16, 1, 36850): (99360, 2305)}


def test_regimes_of_route_1_are_pinned():
    """R is not monotonic in K: it shrinks to stay inside 52 KiB, then starts again at the largest that fits 150 KiB"""
    for (U, D), rows in REGIMES.items():
        assert ref.regimes(U, D) == rows, (U, D)
        for (K, R, pas, route), nxt in zip(rows, rows[1:] + [(2 ** 20 + 1,)]):
            for k in (K, (K + nxt[0]) // 2, nxt[0] - 1):  # the bisection of ref.regimes against the rule itself
                assert (ref.periods_per_lane(k, U, D), ref.route(k, U, D)) == (R, route) and ref.lane_pass(k, U, D) == (R, pas), (U, D, k)
            if R:
                limit = ref.LDS_WANT if pas == 1 else ref.LDS_MAX
                assert ref.lds_elems(R, nxt[0] - 1, U, D) * 8 <= limit
                assert pas == 1 or ref.lds_elems(R, K, U, D) * 8 > ref.LDS_WANT
    for (U, D, K), (nbytes, Wp) in TILES.items():
        assert (ref.lds_elems(ref.periods_per_lane(K, U, D), K, U, D) * 8, ref.window(K, U, D)) == (nbytes, Wp)


def emu_upfirdn(*args, timeout=600):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_upfirdn"), "-s"])
    return subprocess.run([os.path.join(ROOT, "tests", "_build", "emu_upfirdn"), *args], capture_output=True, text=True, timeout=timeout)


def test_restatement_agrees_with_the_device_headers():
    """upfirdn_route, upfirdn_r, upfirdn_lds_elems and upfirdn_window as the headers compute them (tests/emu_upfirdn --geometry), at
    every pinned K and its two neighbours, at the shapes of the other tests and at ratios route 1 does not take"""
    shapes = [(U, D, k) for (U, D), rows in REGIMES.items() for row in rows for k in (row[0] - 1, row[0], row[0] + 1) if k >= 1]
    shapes += SHAPES + [(U, D, K) for U, D in [(65536, 65535), (65536, 2 ** 31 - 1), (65536, 1), (17, 1), (6, 4), (1, 1)]
                        for K in (1, 70, 200000, 2 ** 20, 2 ** 20 + 1, 2 ** 24)]
    out = emu_upfirdn("--geometry", *[str(v) for s in shapes for v in s])
    assert out.returncode == 0, out.stderr
    lines = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(lines) == len(shapes)
    for (U, D, K), line in zip(shapes, lines):
        R = ref.periods_per_lane(K, U, D)
        assert line == (U, D, K, ref.route(K, U, D), R, ref.lds_elems(R, K, U, D) if R else 0, ref.window(K, U, D)), (U, D, K)


def stream_split(hist, W, H, n):
    """libredio_amd/csrc/stream_split.h restated"""
    nh = head_in = nb = off = body_in = 0
    avail = hist + min(n, W - 1)
    if hist > 0 and avail >= W:
        nh = min((hist + H - 1) // H, (avail - W) // H + 1)
        head_in = (nh - 1) * H + W
    start = nh * H
    if start >= hist:
        off = start - hist
        if n >= off + W:
            nb = (n - off - W) // H + 1
            body_in = (nb - 1) * H + W
    return nh, head_in, nb, off, body_in


@pytest.mark.parametrize("U,D,K", [(2, 1, 63), (3, 2, 64), (16, 1, 255), (17, 1, 40), (5, 1, 3), (2, 7, 9), (6, 4, 50), (160, 147, 481)])
def test_stream_segmentation_in_periods(oracle, U, D, K):
    """random cuts on stream_split with (Wp, D', U'): the emitted periods, each computed from its own window by the reference, are the
    prefix of the one-call result; a stateless call on a body has MORE outputs than its periods when U > D, which the stream never writes"""
    rng = np.random.default_rng(SEED + U + K)
    Up, Dp = ref.periods(U, D)
    Wp = ref.window(K, U, D)
    taps = oracle.synth_f32(5, K, K)
    extra_seen = 0
    for trial in range(6):
        N = int(rng.integers(Wp, 40 * Wp + 50 * Dp))
        x = oracle.synth_f32(SEED, trial, N)
        whole = ref.upfirdn(x, taps, U, D)
        hist, skip, pos, emitted = 0, 0, 0, []
        tail = x[:0]
        while pos < N:
            n = min(N - pos, int(rng.choice([0, 1, 2, Wp - 1, Wp, Wp + 1, int(rng.integers(0, 4 * Wp + 3 * Dp)), int(rng.integers(0, 40 * Dp + 2))])))
            new = x[pos: pos + n]
            pos += n
            drop = min(skip, n)
            new, skip = new[drop:], skip - drop
            if len(new) == 0:
                continue
            nh, head_in, nb, off, body_in = stream_split(hist, Wp, Dp, len(new))
            staged = np.concatenate([tail, new])
            if nh:
                emitted.append(ref.upfirdn(staged[:head_in], taps, U, D, count=nh * Up))
            if nb:
                body = new[off: off + body_in]
                emitted.append(ref.upfirdn(body, taps, U, D, count=nb * Up))
                extra_seen = max(extra_seen, ref.nout(len(body), K, U, D) - nb * Up)
                assert ref.nout(len(body), K, U, D) >= nb * Up
            consumed = (nh + nb) * Dp
            if consumed >= len(staged):
                tail, skip = x[:0], consumed - len(staged)
            else:
                tail = staged[consumed:]
            hist = len(tail)
            assert hist < Wp or Wp == 1
        got = np.concatenate(emitted) if emitted else x[:0]
        want_n = Up * ((N - Wp) // Dp + 1)
        assert len(got) == want_n <= len(whole)
        assert np.array_equal(bits(got), bits(whole[:want_n]))
    if (U, D, K) in ((16, 1, 255), (5, 1, 3), (17, 1, 40)):
        assert extra_seen == {(16, 1, 255): 2, (5, 1, 3): 3, (17, 1, 40): 12}[(U, D, K)]


def test_kernels_emulated_thread_by_thread():
    """every route-1 shape at n just under, at and just over one tile and at a last partial tile, aligned and one sample off, real and
    complex, both folds; the direct kernel's thread function on the same calls and on the route-2 shapes; fences intact"""
    out = emu_upfirdn()
    assert out.returncode == 0 and out.stdout.strip().endswith("emu_upfirdn ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_kernels_emulated_thread_by_thread_at_long_filters():
    """the second pass of upfirdn_r at each R (2/1 at 11776 taps: R 4; 3/2 at 36864: R 2; 2/1 at 25396: R 1), the last tap counts
    route 1 takes at 2/1 and 3/8 (36863, 43013) and the direct form one tap later: one whole tile and a partial one, real and complex,
    both folds, aligned and one sample off; the image and the output tile each between fences of their own"""
    out = emu_upfirdn("--long")
    assert out.returncode == 0 and out.stdout.strip().endswith("emu_upfirdn ok"), out.stdout[-2000:] + out.stderr[-2000:]
