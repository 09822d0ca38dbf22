"""The polyphase spectrometer's workgroup kernel (route 2, libredio_amd/csrc/pfb_pspec_p2.hip) without a GPU: its thread programs
behind the transform -- the workgroup's iteration count, the powers, the fold state machine, the stores -- and its stream geometry
(libredio_amd/csrc/pfb_pspec_p2_core.h) emulated on the CPU bit for bit against the restatement (tests/pfb_pspec_ref.py), and the C
ABI of the new symbol."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pfb_pspec_ref as ref
import pspec_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0F5C
SEG = pspec_ref.SEG
P = 4


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def shape_consts(M):
    """streams per workgroup and rows per stream and iteration (pfb_p2_kernel's, the same in both load forms)"""
    return (1, 4096 // M) if M >= 256 else (256 // M, 16)


def unit(u, K, split):
    """(first channelizer row, rows) of unit u: pspec_unit restated"""
    if not split:
        return u * K, K
    S = -(-K // SEG)
    r, s = divmod(u, S)
    return r * K + SEG * s, min(SEG, K - SEG * s)


def units_per_stream(nunits, K, split, cus, M):
    G, _ = shape_consts(M)
    per_unit = SEG if split else K
    return max(-(-nunits // (4 * cus * G)), -(-64 // per_unit))


@pytest.fixture(scope="module")
def emu_p2():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_pspec_p2"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pfb_pspec_p2.so"))
    f32 = np.ctypeslib.ndpointer(np.float32, flags="C")
    c64 = np.ctypeslib.ndpointer(np.complex64, flags="C")
    i32 = np.ctypeslib.ndpointer(np.int32, flags="C")
    i64 = np.ctypeslib.ndpointer(np.int64, flags="C")
    E.emu_pfbspec_p2.argtypes = [c64, C.c_long, C.c_int, C.c_int, C.c_long, C.c_int, C.c_long, C.c_long, C.c_long, f32, i32, i32, i64, i64, C.c_long]
    E.emu_pfbspec_p2.restype = C.c_long
    E.emu_pfbspec_p2_units_per_stream.argtypes = [C.c_long, C.c_long, C.c_int, C.c_long, C.c_int]
    E.emu_pfbspec_p2_units_per_stream.restype = C.c_long
    E.emu_pfbspec_p2_split_rows.argtypes = [C.c_long, C.c_long, C.c_int]
    E.emu_pfbspec_p2_split_rows.restype = C.c_long
    return E


_inputs = {}


def inputs(oracle, M, K):
    """the channelizer's rows and the wanted spectrum, computed once per (M, K): three floor-length runs of output rows and one row more,
    then K - 1 rows of a dropped output row and a few samples"""
    if (M, K) not in _inputs:
        nrows = 3 * -(-64 // K) + 1
        h = oracle.synth_f32(9, P, M * P)
        x = oracle.synth_iq(SEED + K, M, M * (nrows * K + P - 1) + M * (K - 1) + 5)
        assert ref.nrows(len(x), M, P, K) == nrows
        crows = np.ascontiguousarray(ref.channel_rows(x, h, M, P, K))
        want = ref.spectrum(x, h, M, P, K)
        assert crows.shape == (nrows * K, M) and want.shape == (nrows, M)
        crows.setflags(write=False); want.setflags(write=False)
        _inputs[(M, K)] = (nrows, crows, want)
    return _inputs[(M, K)]


def run(emu_p2, crows, M, pair, K, split, nunits, ups, cus):
    G, TR = shape_consts(M)
    used = ups or units_per_stream(nunits, K, split, cus, M)
    nstreams = -(-nunits // used)
    grid = -(-nstreams // G)
    dst = np.full((nunits, M), np.nan, np.float32)
    stores = np.zeros(nunits * M, np.int32)
    owners = np.zeros(nunits, np.int32)
    srows = np.full(2 * grid * G, -1, np.int64)
    giters = np.full(grid, -1, np.int64)
    got = emu_p2.emu_pfbspec_p2(crows, len(crows), M, int(pair), K, int(split), nunits, ups, cus, dst.reshape(-1), stores, owners, srows, giters, grid)
    assert got == grid, (got, grid)
    assert (owners == 1).all(), "every unit is owned by exactly one stream"
    assert (stores == 1).all(), "every element is stored exactly once"
    # the geometry restated: stream s owns units [s used, s used + used), the rows from its first unit's first to its last unit's last,
    # and a workgroup runs as many iterations of TR rows as its longest stream needs
    srows = srows.reshape(grid, G, 2)
    per_stream = np.zeros((grid, G), np.int64)
    for s in range(grid * G):
        u0 = s * used
        if u0 >= nunits:
            want_rows = (len(crows), len(crows))
        else:
            u1 = min(u0 + used, nunits)
            g1, c1 = unit(u1 - 1, K, split)
            want_rows = (unit(u0, K, split)[0], g1 + c1)
        assert tuple(srows[s // G, s % G]) == want_rows, s
        per_stream[s // G, s % G] = -(-(want_rows[1] - want_rows[0]) // TR)
    assert np.array_equal(giters, per_stream.max(axis=1)), "a workgroup's iteration count is the maximum of its streams'"
    return dst, per_stream


FORMS = [(32, False), (256, False), (512, False), (512, True), (1024, False), (1024, True)]


@pytest.mark.parametrize("K", [1, 5, 16, 17, 40])
@pytest.mark.parametrize("M,pair", FORMS)
def test_thread_programs(emu_p2, oracle, M, pair, K):
    """A stream per run of output rows and a stream per run of segments, with the launcher's own run length on a device of one CU
    (the floor: four streams, the last one a single row; at 32 channels half of the workgroup's streams own nothing) and with runs of
    1 and 3 units, which end inside an iteration and, by segments with K > 16, start in the middle of an output row."""
    nrows, crows, want = inputs(oracle, M, K)
    for ups in (0, 1, 3):
        out, _ = run(emu_p2, crows, M, pair, K, False, nrows, ups, 1)
        assert np.array_equal(bits(out), bits(want)), ups
    S = -(-K // SEG)
    ragged = False
    for ups in (0, 1, 3):
        part, per_stream = run(emu_p2, crows, M, pair, K, True, nrows * S, ups, 1)
        part = part.reshape(nrows, S, M)
        folded = part[:, 0].copy()
        for s in range(1, S):
            folded = folded + part[:, s]  # pspec_fold_thread's order
        assert np.array_equal(bits(folded), bits(want)), ups
        owning = per_stream.reshape(-1)[: -(-nrows * S // (ups or units_per_stream(nrows * S, K, True, 1, M))) - 1]  # but the last, short one
        G = per_stream.shape[1]
        ragged = ragged or any(len(set(owning[i: i + G])) > 1 for i in range(0, len(owning), G))
    if M == 32 and K > SEG:
        assert ragged, "by segments the streams of one workgroup differ in their iteration counts"


@pytest.mark.parametrize("M", [32, 128, 256, 512, 1024])
def test_launch_numbers(emu_p2, M):
    """units per stream and the auto rule's row count, restated: 4 cus G streams, at least 64 rows of full units; rows mode from two
    workgroups of floor-length runs per CU"""
    G, _ = shape_consts(M)
    for cus in (1, 8, 256, 304):
        for K in (1, 5, 16, 17, 40, 1024):
            for split in (False, True):
                for nunits in (1, 7, 4 * cus * G * 70, 4 * cus * G * 70 + 1, 10 ** 7):
                    assert emu_p2.emu_pfbspec_p2_units_per_stream(nunits, K, split, cus, M) == units_per_stream(nunits, K, split, cus, M)
            assert emu_p2.emu_pfbspec_p2_split_rows(K, cus, M) == 2 * cus * G * -(-64 // K)


def test_abi(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert hasattr(L, "redio_pfb_pspec_route"), "libredio.so does not export redio_pfb_pspec_route"
    assert "redio_pfb_pspec_route(" in hdr and "#define REDIO_PFB_PSPEC_BLOCK 4u" in hdr
    R = redio.lib()
    assert R.redio_pfb_pspec_route(None) == 0
    assert redio.PolyphaseSpectrum.BLOCK == 2 and (redio.PolyphaseSpectrum.GENERIC, redio.PolyphaseSpectrum.WAVE) == (0, 1)
    p = C.c_void_p()
    taps = (C.c_float * 1024)(*([0.5] * 1024))
    # the flag changes no argument check
    assert R.redio_pfb_pspec_create(None, taps, 128, 8, 4, 4) == -1 and R.redio_pfb_pspec_create(C.byref(p), taps, 128, 8, 0, 4) == -1
    assert R.redio_pfb_pspec_create(C.byref(p), None, 128, 8, 4, 4) == -1 and not p.value
