"""The tuned resampler (redio_ddc_upfirdn_*) without a GPU: the kernels emulated thread by thread on the CPU (tests/emu_ddc_upfirdn, the
device's own headers) against the contract written out -- at the shapes of the GPU tests and at long filters, where the tile is 52 to
150 KiB and the table reads are the longest; the reference (tests/ddc_upfirdn_ref.py) against the oracle's FIR on the zero-stuffed mixed
stream; the bound on a lane's table index over every regime of route 1's geometry; and the stream's segmentation in periods, with the
index that becomes first_index, against a model."""
import os
import subprocess

import numpy as np
import pytest

import ddc_ref
import ddc_upfirdn_ref as ref
import upfirdn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED17D0

# (U, D, K): the twelve shapes of tests/emu_ddc_upfirdn and tests/test_gpu_ddc_upfirdn.py
ROUTE1 = [(2, 1, 63), (3, 2, 64), (2, 3, 31), (4, 5, 100), (3, 8, 17), (7, 10, 40), (6, 4, 50), (5, 1, 3), (1, 5, 127)]
ROUTE2 = [(160, 147, 481), (3, 16, 33), (2, 7, 9)]
SHAPES = ROUTE1 + ROUTE2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def emu(*args, timeout=600):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_ddc_upfirdn"), "-s"])
    return subprocess.run([os.path.join(ROOT, "tests", "_build", "emu_ddc_upfirdn"), *args], capture_output=True, text=True, timeout=timeout)


def test_kernels_emulated_thread_by_thread():
    """the twelve shapes at n just under, at and just over one tile and at a last partial tile, both folds, from cf32 and from bytes;
    periods 1, 2, 3, 24, 65536 times first in {0, 1, L - 1, 2^32 + 5, 2^64 - 1 - n}; every stream and output alignment; the direct
    kernel's thread function on the same calls; every fence intact"""
    out = emu()
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("emu_ddc_upfirdn ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_kernels_emulated_thread_by_thread_at_long_filters():
    """one route-1 shape per R whose tile lies between 52 and 150 KiB (2/1 at 11776 taps: R 4; 3/2 at 36864: R 2; 2/1 at 25396: R 1)
    and the last tap counts route 1 takes at 2/1 and 3/8: one whole tile and a partial one -- the longest table reads"""
    out = emu("--long")
    assert out.returncode == 0 and out.stdout.strip().splitlines()[-1].startswith("emu_ddc_upfirdn ok"), out.stdout[-2000:] + out.stderr[-2000:]


def test_routes_are_the_resamplers():
    for U, D, K in ROUTE1:
        assert ref.route(K, U, D) == 1
    for U, D, K in ROUTE2:
        assert ref.route(K, U, D) == 2 and ref.tile_out(K, U, D) == 256


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("U,D,K", SHAPES)
def test_reference_equals_the_fir_on_the_zero_stuffed_mixed_stream(oracle, U, D, K, fused, u8):
    """finite synthetic input, where skipping a stuffed zero and multiplying it agree"""
    L, first = 24, 2 ** 40 + 3
    w, taps = oracle.synth_iq(7, L, L), oracle.synth_f32(3, K, K)
    for n in [0, 1, 17, 1000, 4099]:
        raw = np.random.default_rng(SEED + n).integers(0, 256, 2 * n, dtype=np.uint8)
        x = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, U + D, n)
        got = ref.ddc_upfirdn_u8(raw, w, taps, U, D, fused, first) if u8 else ref.ddc_upfirdn(x, w, taps, U, D, fused, first)
        want = oracle.fir(upfirdn_ref.zero_stuffed(ddc_ref.mixed(x, w, first), U), taps, D, fused)
        assert got.dtype == want.dtype == np.complex64 and got.shape == want.shape == (ref.nout(n, K, U, D),)
        assert np.array_equal(bits(got), bits(want)), n


def test_a_lanes_table_index_stays_inside_the_extended_table():
    """tile_in + 2 <= DDC_TABLE_EXT at the last tap count of every regime of route 1 (the tile only grows with the taps inside one)"""
    seen = 0
    for U, D in sorted({(U, D) for U, D, K in ROUTE1}):
        rows = upfirdn_ref.regimes(U, D)
        for (K, R, pas, route), nxt in zip(rows, rows[1:] + [(2 ** 20 + 1,)]):
            if route != 1:
                continue
            for k in (K, nxt[0] - 1):
                assert upfirdn_ref.periods_per_lane(k, U, D) == R
                assert ref.tile_in(k, U, D) + 2 <= ref.TABLE_EXT == 20480, (U, D, k)
                assert ref.tile_in(k, U, D) <= upfirdn_ref.lds_elems(R, k, U, D) <= upfirdn_ref.LDS_MAX // 8  # why it holds: the image is in LDS
                seen += 1
    assert seen >= 2 * 3 * len(ROUTE1)


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


@pytest.mark.parametrize("U,D,K", [(2, 1, 63), (3, 2, 64), (5, 1, 3), (2, 7, 9), (6, 4, 50), (160, 147, 481)])
def test_stream_segmentation_in_periods_with_the_index(oracle, U, D, K):
    """random cuts on stream_split with (Wp, D', U'), as stream_carry.hip runs them: every head and body run is a stateless call on its
    own window with first_index = the stream index of the window's first sample (stream_head_first / stream_body_first); the emitted
    periods are the prefix of the one-call result with first_index 0; the index is the count of samples fed"""
    rng = np.random.default_rng(SEED + U + K)
    Up, Dp = ref.periods(U, D)
    Wp = ref.window(K, U, D)
    L = 7 if K % 2 else 24
    w, taps = oracle.synth_iq(9, L, L), oracle.synth_f32(5, K, K)
    for trial in range(4):
        N = int(rng.integers(Wp, 40 * Wp + 50 * Dp))
        x = oracle.synth_iq(SEED, trial, N)
        whole = ref.ddc_upfirdn(x, w, taps, U, D)
        hist, skip, pos, total_in, emitted = 0, 0, 0, 0, []
        tail = x[:0]
        while pos < N:
            n = min(N - pos, int(rng.choice([0, 1, 2, Wp - 1, Wp, Wp + 1, int(rng.integers(0, 4 * Wp + 3 * Dp)), int(rng.integers(0, 40 * Dp + 2))])))
            new = x[pos: pos + n]
            pos += n
            drop = min(skip, n)
            new, skip = new[drop:], skip - drop
            if len(new) == 0:
                total_in += n
                continue
            nh, head_in, nb, off, body_in = stream_split(hist, Wp, Dp, len(new))
            staged = np.concatenate([tail, new])
            if nh:
                first = total_in - hist
                assert first % Dp == 0 and np.array_equal(staged[:head_in], x[first: first + head_in])
                emitted.append(ref.ddc_upfirdn(staged[:head_in], w, taps, U, D, first=first, count=nh * Up))
            if nb:
                first = total_in + drop + off
                assert first % Dp == 0 and np.array_equal(new[off: off + body_in], x[first: first + body_in])
                emitted.append(ref.ddc_upfirdn(new[off: off + body_in], w, taps, U, D, first=first, count=nb * Up))
            consumed = (nh + nb) * Dp
            if consumed >= len(staged):
                tail, skip = x[:0], consumed - len(staged)
            else:
                tail = staged[consumed:]
            hist = len(tail)
            total_in += n
            assert total_in == pos and (hist < Wp or Wp == 1)
        got = np.concatenate(emitted) if emitted else x[:0]
        want_n = Up * ((N - Wp) // Dp + 1)
        assert len(got) == want_n <= len(whole)
        assert np.array_equal(bits(got), bits(whole[:want_n]))
