"""The oversampled channelizer without a GPU: the restatement (tests/pfb_os_ref.py: oracle.fir, np.roll, oracle.fft) against
oracle.pfb_channelizer at hop = nchan and against a float64 evaluation of the defining sum; the ref's stream model; both kernels
(libredio_amd/csrc/pfb_os_core.h) emulated thread by thread by a stand-alone program that fences every index and compares with the
ref's rows bit for bit; the C ABI of the new symbols."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_os_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0532
BOUND = 2e-6  # relative L2 of a transform against float64 (the restatement measured 0.9 - 1.1e-7 of the largest value)
SHAPES = [(64, 4, 64), (64, 4, 32), (64, 4, 16), (64, 4, 48), (32, 3, 20), (12, 2, 5)]
ROWS = [1, 15, 16, 17, 63, 64, 65, 257, 529]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def formula_f64(x, h, M, H, F, rows):
    """X_r[k] = sum_n h[n] x[r H + n] W^(k ((F + r) H + n)), W = e^(-2 pi i / M), in float64; the exponent is reduced mod M exactly"""
    n = np.arange(len(h))
    k = np.arange(M)
    out = np.empty((rows, M), np.complex128)
    for r in range(rows):
        e = (((F + r) * H) % M + n) % M
        Wm = np.exp(-2j * np.pi * ((k[:, None] * e[None, :]) % M) / M)
        out[r] = Wm @ (h.astype(np.float64) * x[r * H: r * H + len(h)].astype(np.complex128))
    return out


def test_nrows_route_and_geometry_laws():
    assert [ref.nrows(n, 64, 4, 32) for n in (0, 255, 256, 287, 288, 256 + 32 * 9)] == [0, 0, 1, 1, 2, 10]
    assert [ref.nrows(n, 12, 2, 5) for n in (23, 24, 28, 29)] == [0, 1, 1, 2]
    assert [ref.route(64, p, 32) for p in (4, 5, 8, 16, 32)] == [1, 0, 1, 1, 0]
    assert ref.route(64, 16, 16) == ref.route(64, 16, 64) == ref.route(32, 8, 16) == 0
    assert [ref.rows_per_wave(r) for r in (1, 64, 65, 2048 * 64, 2048 * 64 + 17, 2 ** 22)] == [64, 64, 64, 64, 80, 2048]
    assert [ref.waves(r) for r in (1, 64, 65, 257, 529, 2048 * 64, 2048 * 64 + 17)] == [1, 1, 2, 5, 9, 2048, 1639]
    assert [ref.shift(F, 0, 64, 32) for F in (0, 1, 2, 2 ** 64 - 530)] == [0, 32, 0, 0]
    assert sorted({ref.shift(0, r, 12, 5) for r in range(24)}) == list(range(12))  # M / gcd(M, H) distinct values


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", [(64, 16), (64, 4), (32, 8), (12, 3)])
def test_at_hop_nchan_the_ref_is_the_channelizer(oracle, M, P, fused):
    x = oracle.synth_iq(SEED, M, (P + 20) * M + 5)
    h = oracle.synth_f32(3, P, M * P)
    want = oracle.pfb_channelizer(x, h, M, P, fused)
    for F in (0, 3):
        got = ref.channelize(x, h, M, P, M, F, fused)
        assert got.shape == want.shape == (21, M) and np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("F", [0, 1, 3])
@pytest.mark.parametrize("M,P,H", SHAPES)
def test_ref_against_the_float64_formula(oracle, M, P, H, F):
    rows = 23
    x = oracle.synth_iq(SEED, M + H, M * P + (rows - 1) * H + H - 1)
    h = oracle.synth_f32(3, P, M * P)
    got = ref.channelize(x, h, M, P, H, F)
    assert got.shape == (rows, M) == (ref.nrows(len(x), M, P, H), M)
    want = formula_f64(x, h, M, H, F, rows)
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"{M}x{P} hop {H} F={F}: relative L2 {err:.3e}")
    assert err <= BOUND


@pytest.mark.parametrize("M,P,H", [(64, 4, 32), (64, 4, 48), (12, 2, 5)])
def test_stream_model_does_not_depend_on_the_split(oracle, M, P, H):
    n = M * P + 37 * H + 3
    x = oracle.synth_iq(SEED, 7, n)
    h = oracle.synth_f32(3, 1, M * P)
    want = ref.channelize(x, h, M, P, H).reshape(-1)
    rng = np.random.default_rng(SEED + H)
    for cuts in ([n], [1] * 40 + [n - 40], [M * P - 1, 1, H - 1, 1, n - M * P - H], [0, 31, 0, 33, n - 64],
                 list(rng.multinomial(n, np.ones(9) / 9))):
        assert sum(cuts) == n
        s, got, at = ref.StreamModel(h, M, P, H), [], 0
        for c in cuts:
            assert s.nout(c) == ref.nrows(s.pending + c, M, P, H) * M
            got.append(s.feed(x[at: at + c]))
            assert len(got[-1]) % M == 0 and s.pending < M * P
            at += c
        got = np.concatenate(got)
        assert np.array_equal(bits(got), bits(want)) and s.row == ref.nrows(n, M, P, H) and s.pending == n - s.row * H
    s.reset()
    assert s.pending == 0 and s.row == 0


def emu(*args, san=False):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_os"), "-s"] + (["san"] if san else []))
    exe = os.path.join(ROOT, "tests", "_build", "emu_pfb_os_san" if san else "emu_pfb_os")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stderr)
    return int(r.stdout)


@functools.lru_cache(maxsize=None)
def wave_case(P, fused):
    """the longest stream of the wave-kernel cases and its branch sums, computed once: every shorter case is a prefix"""
    import oracle
    x = oracle.synth_iq(SEED, P, 64 * P + 32 * (max(ROWS) - 1))
    h = oracle.synth_f32(3, 64 * P, 64 * P)
    u = ref.branch_sums(x, h, 64, P, 32, fused)
    for a in (x, h, u):
        a.setflags(write=False)
    return x, h, u


def rows_from(u, rows, M, H, F):
    import oracle
    v = ref.roll_rows(u[:rows], M, H, F)
    return v, oracle.fft(np.ascontiguousarray(v.reshape(-1)), M, inverse=False).reshape(rows, M)


def run_wave_cases(tmp_path, P, fused, rows_list, san=False):
    x, h, u = wave_case(P, fused)
    i, t, w = (str(tmp_path / n) for n in ("in.bin", "taps.bin", "want.bin"))
    h.tofile(t)
    for rows in rows_list:
        x[: 64 * P + 32 * (rows - 1)].tofile(i)
        for F in (0, 1, 2 ** 64 - 1 - rows):
            rows_from(u, rows, 64, 32, F)[1].tofile(w)
            assert emu("wave", P, int(fused), rows, F, i, t, w, san=san) == ref.waves(rows)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_wave_kernel_emulated_wavefront_by_wavefront(oracle, tmp_path, P, fused):
    """every lane of every wavefront under the launcher's geometry, F even, odd and 2^64 - 1 - rows; the program fences every load,
    LDS index and store, wants every output written once, and compares with the ref's rows bit for bit"""
    x, h, u = wave_case(P, fused)
    assert np.array_equal(bits(rows_from(u, 65, 64, 32, 1)[1]), bits(ref.channelize(x[: 64 * P + 32 * 64], h, 64, P, 32, 1, fused)))
    run_wave_cases(tmp_path, P, fused, ROWS)


BRANCH_CASES = [(64, 16, 16, 40, 7), (64, 5, 32, 40, 40), (64, 8, 48, 43, 5), (32, 8, 16, 40, 40), (256, 4, 128, 9, 4), (12, 3, 5, 43, 5),
                (100, 2, 100, 40, 40), (64, 4, 32, 529, 100)]


@pytest.mark.parametrize("fused", [False, True])
def test_branch_pass_emulated_thread_by_thread(oracle, tmp_path, fused):
    """route 0's first pass: the loads, the shift and the rotated store of every thread, in passes as the plan cuts them"""
    i, t, w = (str(tmp_path / n) for n in ("in.bin", "taps.bin", "want.bin"))
    for M, P, H, rows, chunk in BRANCH_CASES:
        x = oracle.synth_iq(SEED, M, M * P + H * (rows - 1))
        h = oracle.synth_f32(3, M, M * P)
        x.tofile(i)
        h.tofile(t)
        for F in (0, 3, 2 ** 64 - 1 - rows):
            ref.rotated(x, h, M, P, H, F, fused).tofile(w)
            assert emu("branch", M, P, H, int(fused), rows, F, chunk, i, t, w) == -(-rows // chunk)


def test_emulation_under_sanitizers(oracle, tmp_path):
    """the same program built with -fsanitize=address,undefined and run directly: a plain host program, nothing to preload"""
    run_wave_cases(tmp_path, 8, True, [17, 65], san=True)
    run_wave_cases(tmp_path, 16, False, [65], san=True)
    M, P, H, rows = 12, 3, 5, 43
    x, h = oracle.synth_iq(SEED, M, M * P + H * (rows - 1)), oracle.synth_f32(3, M, M * P)
    i, t, w = (str(tmp_path / n) for n in ("bin.bin", "btaps.bin", "bwant.bin"))
    x.tofile(i)
    h.tofile(t)
    ref.rotated(x, h, M, P, H, 3, True).tofile(w)
    assert emu("branch", M, P, H, 1, rows, 3, 5, i, t, w, san=True) == 9


def test_emulation_rejects_wrong_rows(oracle, tmp_path):
    """the program's comparison is live: rows for another F fail it"""
    x, h, u = wave_case(4, False)
    i, t, w = (str(tmp_path / n) for n in ("in.bin", "taps.bin", "want.bin"))
    x[: 256 + 32 * 16].tofile(i)
    h.tofile(t)
    rows_from(u, 17, 64, 32, 1)[1].tofile(w)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_os"), "-s"])
    r = subprocess.run([os.path.join(ROOT, "tests", "_build", "emu_pfb_os"), "wave", "4", "0", "17", "0", i, t, w], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "same_bits" in r.stderr


NAMES = ["redio_pfb_os_" + n for n in ("create", "destroy", "nrows", "hop", "route", "is_fused", "set_unfused", "set_chunk_rows", "reserve", "enqueue")] + [
    f"redio_pfb_os_stream_{s}" for s in ("create", "destroy", "reset", "nout", "pending", "enqueue")]


def test_header_and_exports(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_pfb_os redio_pfb_os;" in hdr and "typedef struct redio_pfb_os_stream redio_pfb_os_stream;" in hdr
    declared = set(re.findall(r"\b(redio_pfb_os\w*)\(", hdr))
    assert declared == set(NAMES)
    for n in sorted(declared):
        assert hasattr(L, n), f"libredio.so does not export {n}"
    assert hasattr(redio, "OversampledChannelizer") and issubclass(redio.OversampledChannelizerStream, redio.Stream)
