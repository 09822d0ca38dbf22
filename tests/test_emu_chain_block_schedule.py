"""The chain kernel transforms block b under the FIR of block b + 1 with each of the transform's two LDS exchanges done in two
halves (libredio_amd/csrc/fft_core.h: fft1kn_x1h_*, fft1kn_x2h_*; fft_wave.h: fft1kn_wave_piece).  By enumeration on the CPU
(tests/emu_sched): in the one-piece maps and in either half every (lane, element) is written exactly once and read exactly once, a
half stays inside its FFT1KN_HALF_LDS float2, and the halves compose to the one-piece map -- a reader gets, register for register,
the value the one-piece exchange hands it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_sched"), "-s"])
    lib = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_sched.so"))
    pi = C.POINTER(C.c_int)
    lib.emu_sched_consts.argtypes = [pi]
    lib.emu_sched_maps.argtypes = [C.c_int] + [pi] * 6
    lib.emu_sched_maps.restype = C.c_int
    lib.emu_sched_half_of.argtypes = [C.c_int, C.c_int, pi]
    lib.emu_sched_half_of.restype = C.c_int
    return lib


def consts(emu):
    v = np.zeros(5, np.int32)
    emu.emu_sched_consts(v.ctypes.data_as(C.POINTER(C.c_int)))
    return dict(zip(("row1", "row2", "lds", "hrow1", "half_lds"), (int(i) for i in v)))


def maps(emu, x):
    t = [np.full((64, 16), -1, np.int32) for _ in range(6)]
    assert emu.emu_sched_maps(x, *[a.ctypes.data_as(C.POINTER(C.c_int)) for a in t]) == 0
    return dict(zip(("store1", "load1", "store_half", "store_h", "load_half", "load_h"), t))


def test_half_exchange_fits_behind_the_image(emu):
    c = consts(emu)
    assert c["lds"] == 16 * c["row1"] and c["half_lds"] == 16 * c["hrow1"]
    assert c["half_lds"] >= 8 * c["row2"], "the second exchange's eight rows fit the same area"
    image = 1542  # FirGeomV<127, 5, 4>::lds_elems(256): 1402 samples, two pad elements per 20
    assert (image + c["half_lds"] + 60) * 8 <= 160 * 1024 // 8 - 480, "image + half exchange + twiddle table within a wave's request"
    assert (image + c["lds"]) * 8 > 160 * 1024 // 8 - 480, "a one-piece exchange beside the image would not fit"


@pytest.mark.parametrize("x", [1, 2])
def test_one_piece_map_is_a_permutation(emu, x):
    c, m = consts(emu), maps(emu, x)
    st, ld = m["store1"].ravel(), m["load1"].ravel()
    assert st.min() >= 0 and st.max() < c["lds"]
    assert len(np.unique(st)) == 1024, "every (lane, element) written to a place of its own"
    assert np.array_equal(np.sort(ld), np.sort(st)), "every written place read exactly once"


@pytest.mark.parametrize("x", [1, 2])
def test_each_half_written_once_and_read_once(emu, x):
    c, m = consts(emu), maps(emu, x)
    assert set(np.unique(m["store_half"])) == {0, 1} and set(np.unique(m["load_half"])) == {0, 1}
    for h in (0, 1):
        st = m["store_h"][m["store_half"] == h]
        ld = m["load_h"][m["load_half"] == h]
        assert st.size == 512 and ld.size == 512, "half of the 1024 values each"
        assert st.min() >= 0 and st.max() < c["half_lds"]
        assert len(np.unique(st)) == 512, "written exactly once"
        assert np.array_equal(np.sort(ld), np.sort(st)), "read exactly once"
    # the split keeps every read at full width: a lane reads eight elements in either half
    assert np.all((m["load_half"] == 0).sum(axis=1) == 8)
    # ... and a lane stores all sixteen of its values in one half
    assert np.all(m["store_half"].min(axis=1) == m["store_half"].max(axis=1))
    assert np.all(np.bincount(m["store_half"][:, 0], minlength=2) == 32)


@pytest.mark.parametrize("x", [1, 2])
def test_halves_compose_to_the_one_piece_map(emu, x):
    m = maps(emu, x)
    half = C.c_int(-1)
    for side in ("store", "load"):
        one, hh, hi = m[side + "1"], m[side + "_half"], m[side + "_h"]
        for lane in range(64):
            for i in range(16):
                idx = emu.emu_sched_half_of(x, int(one[lane, i]), C.byref(half))
                assert (half.value, idx) == (int(hh[lane, i]), int(hi[lane, i])), (side, lane, i)
    # so the writer whose value lane l reads into register i is the one-piece exchange's: same (half, place) on both sides
    src1 = {int(a): (l, i) for (l, i), a in np.ndenumerate(m["store1"])}
    srch = {(int(m["store_half"][l, i]), int(a)): (l, i) for (l, i), a in np.ndenumerate(m["store_h"])}
    for (l, i), a in np.ndenumerate(m["load1"]):
        assert srch[(int(m["load_half"][l, i]), int(m["load_h"][l, i]))] == src1[int(a)]
