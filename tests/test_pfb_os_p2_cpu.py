"""The oversampled channelizer's workgroup kernel (route 2, libredio_amd/csrc/pfb_os_p2.hip) without a GPU: the front of its thread
programs -- stream geometry, the clamped loads, the two windows and their rotation, both folds, the store into the image -- emulated on
the CPU through libredio_amd/csrc/pfb_os_p2_core.h, bit for bit against the restatement (tests/pfb_os_ref.rotated); the route rule,
the flag and the C ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_os_p2_ref as p2
import pfb_os_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_os_p2"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pfb_os_p2.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    i64 = np.ctypeslib.ndpointer(np.int64, flags="C")
    E.emu_pfb_os_p2.argtypes = [c64, C.c_long, f32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_long, C.c_uint64, C.c_long, C.c_long, c64, i32, i64, C.c_long]
    E.emu_pfb_os_p2.restype = C.c_long
    E.emu_pfb_os_p2_rows_per_stream.argtypes = [C.c_long, C.c_long, C.c_int]
    E.emu_pfb_os_p2_rows_per_stream.restype = C.c_long
    return E


def run(emu, M, P, pair, fused, rows, F, cus, rps):
    """one emulated launch; the image rows put back into channel order"""
    x, h, _ = p2.case(M, P, fused)
    n = p2.n_in(M, P, rows)
    G, TR = p2.shape_consts(M)
    used = rps or p2.rows_per_stream(rows, cus, M)
    streams = -(-rows // used)
    grid = -(-streams // G)
    img = np.full((rows, M), np.nan, np.complex64)
    stores = np.zeros(rows * M, np.int32)
    geom = np.zeros(3, np.int64)
    # x holds M / 2 - 1 samples more than the call may read: the fence is at n
    got = emu.emu_pfb_os_p2(x, n, h, M, P, int(pair), int(fused), rows, F, cus, rps, img.reshape(-1), stores, geom, grid)
    assert got == grid, (got, grid, "negative: -2 a load outside the call's samples, -3 the image, -4 a half-row loaded twice or never")
    assert tuple(geom) == (used, streams, grid)
    assert (stores == 1).all(), "the stored rows cover [0, rows) exactly once"
    order = np.array([p2.leaf_pos(k, M) for k in range(M)])
    return img[:, order], grid


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", p2.ALL_SHAPES)
def test_front_of_the_kernel(emu, M, P, fused):
    """Every shape in every load form it has, every row count of the GPU cases, three first rows: with the launcher's geometry on a
    device of one CU (several workgroups from 64 G + 1 rows on; at 32 and 128 channels streams that own nothing) and with runs of one
    and of three iterations, which put a stream seam into every 16 rows and end on the pair loop's single iteration."""
    G, TR = p2.shape_consts(M)
    several = False
    for pair in ([False, True] if M >= 512 else [False]):
        for rows in p2.rows_list(M):
            if rows == 0:
                assert ref.nrows(p2.n_in(M, P, 0), M, P, M // 2) == 0  # nothing is launched
                continue
            assert ref.nrows(p2.n_in(M, P, rows) + M // 2 - 1, M, P, M // 2) == rows
            for F in (0, 1, 2 ** 64 - 1 - rows):
                want = p2.want_rotated(M, P, fused, F & 1)[:rows]
                for rps in ((0, TR, 3 * TR) if F == 1 else (0,)):
                    got, grid = run(emu, M, P, pair, fused, rows, F, 1, rps)
                    several = several or grid > 1
                    assert np.array_equal(bits(got), bits(want)), (pair, rows, F, rps)
    assert several


def test_the_shared_reference_is_the_contract():
    """the cases share branch sums and take the shift from the parity of F: the same rows as pfb_os_ref.rotated on the call's own input"""
    M, P = 32, 4
    x, h, _ = p2.case(M, P, True)
    for rows in (1, 17, 65):
        for F in (0, 1, 7, 2 ** 64 - 1 - rows):
            want = ref.rotated(x[: p2.n_in(M, P, rows)], h, M, P, M // 2, F, True)
            assert np.array_equal(bits(want), bits(p2.want_rotated(M, P, True, F & 1)[:rows]))


@pytest.mark.parametrize("M", p2.CHANNELS)
def test_launch_numbers(emu, M):
    G, TR = p2.shape_consts(M)
    for cus in (1, 8, 256, 304):
        for rows in (1, 63, 64, 65, 64 * 4 * cus * G, 64 * 4 * cus * G + 1, 10 ** 7):
            rps = emu.emu_pfb_os_p2_rows_per_stream(rows, cus, M)
            assert rps == p2.rows_per_stream(rows, cus, M) and rps % TR == 0 and rps % 2 == 0 and rps >= 64


def test_route_rule():
    """route 2 on the flagged shapes at hop nchan / 2 and only there; without the flag pfb_os_ref.route"""
    two = set()
    for M in (12, 16, 32, 64, 100, 128, 256, 512, 1024, 2048):
        for P in (2, 3, 4, 5, 8, 16, 32):
            for H in {1, M // 4, M // 2, M // 2 + 1, M}:
                assert p2.route(M, P, H, False) == ref.route(M, P, H)
                r = p2.route(M, P, H, True)
                if r == 2:
                    two.add((M, P))
                    assert H == M // 2
                else:
                    assert r == ref.route(M, P, H)
    assert two == set(p2.SHAPES) and len(p2.ALL_SHAPES) == 15 and set(p2.ALL_SHAPES) - two == set(p2.LEFT_OUT)
    assert p2.route(64, 8, 32, True) == 1 and p2.route(256, 8, 64, True) == 0 and p2.route(100, 3, 50, True) == 0


def test_flag_and_abi(redio):
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    m = re.search(r"#define REDIO_PFB_OS_BLOCK (\d+)u", hdr)
    assert m and int(m.group(1)) == redio.REDIO_PFB_OS_BLOCK == 4
    assert (redio.OversampledChannelizer.TWO_PASS, redio.OversampledChannelizer.WAVE, redio.OversampledChannelizer.BLOCK) == (0, 1, 2)
    R = redio.lib()
    assert R.redio_pfb_os_route(None) == 0 and R.redio_pfb_os_is_fused(None) == 0
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    # the flag changes no argument check
    for flags in (4, 6):
        assert R.redio_pfb_os_create(None, taps, 128, 8, 64, flags) == -1
        assert R.redio_pfb_os_create(C.byref(p), None, 128, 8, 64, flags) == -1 and not p.value
        assert R.redio_pfb_os_create(C.byref(p), taps, 128, 8, 0, flags) == -1 and not p.value
        assert R.redio_pfb_os_create(C.byref(p), taps, 128, 8, 129, flags) == -1 and not p.value
