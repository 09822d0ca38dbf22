"""The FIR's chunked tiled kernel without a GPU: the shared plain loader, fir_chunks and the transpose store (libredio_amd/csrc/fir_tile.h,
fir_chunks.h) run for every thread of a workgroup on the CPU (tests/emu_fir), on an image of exactly the allocated elements between fences
of NaN.  Outputs are compared bit for bit with the fold written out (ascending taps; a rounded multiply then a rounded add, or fmaf),
no write may fall outside the image, and nothing but the outputs may be written to y."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = {1: (8, 16), 2: (4, 16), 3: (4, 24), 4: (4, 16), 5: (4, 40), 8: (2, 16), 10: (2, 40)}  # decimation: (outputs per lane, whole-chunk size)
SEED = 0xF1257113


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_fir"), "-s"])
    L = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_fir.so"))
    vp, i, l = C.c_void_p, C.c_int, C.c_long
    L.emu_fir_r.restype = L.emu_fir_chw.restype = i
    L.emu_fir_r.argtypes = L.emu_fir_chw.argtypes = [l]
    L.emu_fir_lds_elems.restype = l
    L.emu_fir_lds_elems.argtypes = [l, l]
    L.emu_fir_lds_max.restype = l
    L.emu_fir_lds_max.argtypes = []
    L.emu_fir_tile.restype = i
    L.emu_fir_tile.argtypes = [i, i, l, i, vp, l, vp, l, vp, l]
    L.emu_fir_fold.restype = None
    L.emu_fir_fold.argtypes = [i, i, l, i, vp, vp, vp, l]
    return L


def test_table_and_allocation_are_the_documented_ones(emu):
    """the table, and the allocation rule restated: four elements past the tile, one pad element per even lane stride, two more, never
    less than the 256 (R + 1) elements of the output transpose; 150 KiB"""
    assert emu.emu_fir_lds_max() == 150 * 1024
    for D in range(1, 20):
        R, chw = TABLE.get(D, (0, 16))
        assert emu.emu_fir_r(D) == R and (not R or emu.emu_fir_chw(D) == chw)
        for K in (1, 15, 16, 17, 300, 4097, 15008, 2 ** 20):
            t, lstr = (256 * R - 1) * D + (K + 15) // 16 * 16 + 4, R * D
            assert emu.emu_fir_lds_elems(K, D) == (max(t + (t // lstr if lstr % 2 == 0 else 0) + 2, 256 * (R + 1)) if R else 0), (K, D)


def last_k(emu, D, size):
    """the largest tap count whose tile fits the budget at `size` bytes per sample (the allocation never shrinks as the taps grow)"""
    lo, hi = 1, 2 ** 20
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if emu.emu_fir_lds_elems(mid, D) * size <= emu.emu_fir_lds_max() else (lo, mid - 1)
    return lo


def offset_view(n, dtype, off):
    """n samples `off` samples behind a 16-byte boundary, inside a buffer of NaN with 64 samples of slack on either side"""
    w = np.dtype(dtype).itemsize // 4
    raw = np.full((n + 160) * w + 8, np.nan, np.float32)
    a = (-raw.ctypes.data // 4) % 4  # floats up to the next 16-byte boundary
    start = a + (64 + off) * w
    return raw, raw[start: start + n * w].view(dtype), start


def run_case(emu, cplx, fused, D, K, x, h, n_out, tiles, xoff, yoff):
    dtype = np.complex64 if cplx else np.float32
    w = 2 if cplx else 1
    _, xv, _ = offset_view(len(x), dtype, xoff)
    xv[:] = x
    yraw, yv, ystart = offset_view(n_out, dtype, yoff)
    assert (xv.ctypes.data % 16 == 0) == (xoff * 4 * w % 16 == 0) and (yv.ctypes.data % 16 == 0) == (yoff * 4 * w % 16 == 0)
    taps = np.zeros((K + 15) // 16 * 16, np.float32)
    taps[:K] = h
    T = 256 * TABLE[D][0]
    for tile in tiles:
        bad = emu.emu_fir_tile(int(cplx), int(fused), D, K, xv.ctypes.data, len(x), taps.ctypes.data, tile, yv.ctypes.data, n_out)
        assert bad == 0, f"{bad} image writes outside the LDS allocation"
    want = np.empty(n_out, dtype)
    emu.emu_fir_fold(int(cplx), int(fused), D, K, xv.ctypes.data, taps.ctypes.data, want.ctypes.data, n_out)
    lo, hi = min(tiles) * T, min(n_out, (max(tiles) + 1) * T)
    assert np.array_equal(bits(yv[lo:hi]), bits(want[lo:hi])), (cplx, fused, D, K, n_out, xoff, yoff)
    touched = ~np.isnan(yraw)
    touched[ystart + lo * w: ystart + hi * w] = False
    assert not touched.any(), "a store outside the tile's outputs"
    return want


def samples(rng, n, cplx):
    v = rng.uniform(-1, 1, n * (2 if cplx else 1)).astype(np.float32)
    return v.view(np.complex64) if cplx else v


@pytest.mark.parametrize("cplx", [False, True], ids=["f32", "cf32"])
@pytest.mark.parametrize("D", sorted(TABLE))
def test_chunked_kernel_emulated(emu, oracle, D, cplx):
    """every tap count around the chunk sizes; inputs that end inside the first tile, exactly on it and one output into the next, the
    shortest input for them (the guarded loops) and one with the whole first tile behind it (the loads in flight); x and y on and off
    the 16-byte grid; both roundings.  The last tap count inside 150 KiB runs one tile, and one tap more is refused."""
    R, CHW = TABLE[D]
    T = 256 * R
    size = 8 if cplx else 4
    rng = np.random.default_rng(SEED + 2 * D + cplx)
    offs = [(0, 0), (1, 0), (0, 1), (1, 1)] if cplx else [(0, 0), (1, 3), (2, 1), (3, 2)]
    case = 0
    for K in sorted({1, 15, 16, 17, CHW - 1, CHW, CHW + 1}):
        h = rng.uniform(-1, 1, K).astype(np.float32)
        for n_out, tiles in [(T // 2 + 3, [0]), (T, [0]), (T + 1, [0, 1])]:
            for slack in (0, 64):  # samples behind the last window: with 64 the first tile exists whole
                x = samples(rng, (n_out - 1) * D + K + slack, cplx)
                for xoff, yoff in offs:
                    fused = bool(case & 1)
                    case += 1
                    want = run_case(emu, cplx, fused, D, K, x, h, n_out, tiles, xoff, yoff)
                    if (xoff, yoff) == (0, 0) and slack == 0:
                        assert np.array_equal(bits(want), bits(oracle.fir(x, h, D, fused)))  # the written-out fold is the oracle's
    K = last_k(emu, D, size)
    assert emu.emu_fir_lds_elems(K, D) * size <= 150 * 1024 < emu.emu_fir_lds_elems(K + 1, D) * size
    h = rng.uniform(-1, 1, K + 1).astype(np.float32)
    for fused, (xoff, yoff), slack in [(False, offs[0], 64), (True, offs[3], 0)]:
        x = samples(rng, (T - 1) * D + K + slack, cplx)
        run_case(emu, cplx, fused, D, K, x, h[:K], T, [0], xoff, yoff)
    taps = np.zeros((K + 16) // 16 * 16, np.float32)
    assert emu.emu_fir_tile(int(cplx), 0, D, K + 1, x.ctypes.data, len(x), taps.ctypes.data, 0, None, 0) == -1


def test_no_chunked_form_off_the_table(emu):
    x = np.zeros(64, np.float32)
    for D in (6, 7, 9, 11, 16):
        assert emu.emu_fir_tile(0, 0, D, 16, x.ctypes.data, 64, x.ctypes.data, 0, None, 0) == -1
