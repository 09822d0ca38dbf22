"""The synthesis filterbank without a GPU: the restatement (tests/pfb_synth_ref.py: one oracle.fft per row, one oracle.fir per branch)
against float64 numpy, through the one-tap round trip with oracle.pfb_channelizer and against the channelizer's own branch filter; the
wave kernel's lane programs (libredio_amd/csrc/pfb_synth_core.h, pfb_core.h with INV = true) emulated wavefront by wavefront by a
stand-alone program, bit for bit against the restatement; a golden file that pins the restatement; the C ABI of the new symbols.
`python tests/test_pfb_synth_cpu.py` rewrites the golden file from the restatement."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_synth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pfb_synth_64x4")
SEED = 0x5EED5176
BOUND = 2e-6  # relative L2 of a transform against float64 (the restatement measured at most 1.2e-7)
SHAPES = [(64, 16), (64, 4), (32, 8), (12, 3), (256, 4)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rel_l2(got, want):
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def synth_f64(X, h, M, P):
    """the contract in float64: numpy's inverse transform without its 1 / M, then the correlation over P rows"""
    V = np.fft.ifft(X.astype(np.complex128).reshape(-1, M), axis=1) * M
    g = h.astype(np.float64).reshape(P, M)
    T = V.shape[0]
    return sum(V[p: T - P + 1 + p] * g[p] for p in range(P)).reshape(-1)


@pytest.mark.parametrize("M,P", [(64, 16), (7, 2), (1, 1)])
def test_nout_and_route_laws(M, P):
    assert ref.nout(P * M - 1, M, P) == 0 and ref.nout(P * M, M, P) == M
    assert ref.nout((P + 1) * M - 1, M, P) == M and ref.nout((P + 9) * M, M, P) == 10 * M
    assert ref.nout(0, M, P) == 0
    assert ref.route(M, P) == (1 if (M, P) == (64, 16) else 0)
    assert [ref.route(64, p) for p in (4, 5, 8, 16, 32)] == [1, 0, 1, 1, 0]


def test_launch_geometry():
    """launch_pfb_t's decision on output rows: runs are a multiple of 16 rows, at least 64, about 2048 waves"""
    assert [ref.rows_per_wave(r) for r in (1, 64, 65, 2048 * 64, 2048 * 64 + 1, 2 ** 22)] == [64, 64, 64, 64, 80, 2048]
    assert [ref.waves(r) for r in (1, 64, 65, 257, 2048 * 64, 2048 * 64 + 1)] == [1, 1, 2, 5, 2048, 1639]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", SHAPES)
def test_ref_against_float64(oracle, M, P, fused):
    x = oracle.synth_iq(SEED, M, (P + 20) * M + 3)
    h = oracle.synth_f32(3, P, M * P)
    got = ref.synth(x, h, M, P, fused)
    want = synth_f64(x[: (P + 20) * M], h, M, P)
    assert len(got) == 21 * M == ref.nout(len(x), M, P)
    err = rel_l2(got, want)
    print(f"{M}x{P} fused={fused}: relative L2 {err:.3e}")
    assert err <= BOUND


@pytest.mark.parametrize("M,P,pa,ps", [(64, 4, 0, 0), (64, 4, 1, 2), (32, 8, 7, 3), (12, 3, 2, 0)])
def test_one_tap_round_trip(oracle, M, P, pa, ps):
    """analysis branches a single 1.0 at tap pa, synthesis branches at ps: synth(channelizer(x))[i] = M x[i + (pa + ps) M]"""
    n = (2 * P + 30) * M
    x = oracle.synth_iq(SEED, 7, n)
    ea, es = np.zeros(M * P, np.float32), np.zeros(M * P, np.float32)
    ea[pa * M: (pa + 1) * M] = 1.0
    es[ps * M: (ps + 1) * M] = 1.0
    got = ref.synth(oracle.pfb_channelizer(x, ea, M, P).reshape(-1), es, M, P)
    d = (pa + ps) * M
    assert len(got) == n - 2 * (P - 1) * M
    err = rel_l2(got, M * x[d: d + len(got)].astype(np.complex128))
    print(f"one-tap round trip {M}x{P}: relative L2 {err:.3e}")
    assert err <= BOUND


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", SHAPES)
def test_the_branch_filter_is_the_channelizers(oracle, M, P, fused):
    """the definition's symmetry: the ref's step 2 on rows V is the channelizer with its forward transform undone -- the forward
    transform of every ref-filtered row is the channelizer's row when V is fed as its input stream, bit for bit"""
    V = oracle.synth_iq(SEED, 3, (P + 9) * M).reshape(-1, M)
    h = oracle.synth_f32(3, P, M * P)
    filtered = ref.filter_rows(V, h, M, P, fused)
    want = oracle.pfb_channelizer(V.reshape(-1), h, M, P, fused)
    got = oracle.fft(filtered.reshape(-1), M, inverse=False).reshape(-1, M)
    assert got.shape == want.shape == (10, M) and np.array_equal(bits(got), bits(want))


def emu(P, fused, rpw, rows, x, h, tmp_path, san=False):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_synth"), "-s"] + (["SAN=1"] if san else []))
    i, t, o = (str(tmp_path / n) for n in ("in.bin", "taps.bin", "out.bin"))
    x.tofile(i)
    h.tofile(t)
    exe = os.path.join(ROOT, "tests", "_build", "emu_pfb_synth_san" if san else "emu_pfb_synth")
    r = subprocess.run([exe, str(P), str(int(fused)), str(rpw), str(rows), i, t, o], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return int(r.stdout), np.fromfile(o, np.complex64)


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_wave_kernel_emulated_wavefront_by_wavefront(oracle, tmp_path, P, fused):
    """runs of 64 and 80 rows and the launcher's own; the last wave's run is cut by t1 and its reads are clamped.  The program checks
    every LDS and global index and that every output is written once; here its output against the ref, bit for bit."""
    h = oracle.synth_f32(3, P, 64 * P)
    for rpw, rows, nwaves in ((64, 64 + 37, 2), (80, 2 * 80 + 5, 3), (64, 128, 2), (0, 1, 1), (0, 70, 2)):
        x = oracle.synth_iq(SEED, rows, (rows + P - 1) * 64)
        n, got = emu(P, fused, rpw, rows, x, h, tmp_path)
        assert n == nwaves == (ref.waves(rows) if rpw == 0 else -(-rows // rpw))
        assert np.array_equal(bits(got), bits(ref.synth(x, h, 64, P, fused))), (rpw, rows)


def test_wave_kernel_emulation_under_sanitizers(oracle, tmp_path):
    """the same program built with -fsanitize=address,undefined: a plain host program, nothing to preload"""
    P, rows = 8, 64 + 37
    h = oracle.synth_f32(3, P, 64 * P)
    x = oracle.synth_iq(SEED, rows, (rows + P - 1) * 64)
    n, got = emu(P, True, 64, rows, x, h, tmp_path, san=True)
    assert n == 2 and np.array_equal(bits(got), bits(ref.synth(x, h, 64, P, True)))


def golden_case(oracle):
    meta = json.load(open(GOLDEN + ".json"))
    M, P = meta["nchan"], meta["taps_per_branch"]
    x = oracle.synth_iq(meta["seed"], meta["first"], (meta["out_rows"] + P - 1) * M)
    h = oracle.synth_f32(meta["taps_seed"], meta["taps_first"], M * P)
    return meta, ref.synth(x, h, M, P, meta["fused"]).reshape(meta["out_rows"], M)


def test_golden_file_pins_the_ref(oracle):
    meta, got = golden_case(oracle)
    want = np.load(GOLDEN + ".npy")
    assert (meta["nchan"], meta["taps_per_branch"], meta["out_rows"]) == (64, 4, 8)
    assert want.dtype == np.complex64 and want.shape == got.shape == (8, 64)
    assert np.array_equal(bits(got), bits(want))


NAMES = ["redio_pfb_synth_" + n for n in ("create", "destroy", "nout", "route", "is_fused", "set_unfused", "set_chunk_rows", "reserve", "enqueue")] + [
    f"redio_pfb_synth_stream_{s}" for s in ("create", "destroy", "reset", "nout", "pending", "enqueue")]


def test_header_and_exports(redio):
    L = C.CDLL(redio.LIBREDIO)
    hdr = open(os.path.join(ROOT, "include", "redio.h")).read()
    assert "typedef struct redio_pfb_synth redio_pfb_synth;" in hdr and "typedef struct redio_pfb_synth_stream redio_pfb_synth_stream;" in hdr
    declared = set(re.findall(r"\b(redio_pfb_synth\w*)\(", hdr))
    assert declared == set(NAMES)
    for n in sorted(declared):
        assert hasattr(L, n), f"libredio.so does not export {n}"
    assert "inverse transform, then the same branch filter" in hdr


if __name__ == "__main__":
    import sys
    sys.path.insert(0, ROOT)
    import oracle as O
    json.dump({"nchan": 64, "taps_per_branch": 4, "fused": False, "out_rows": 8, "seed": SEED, "first": 0, "taps_seed": 3, "taps_first": 0,
               "input": "oracle.synth_iq(seed, first, (out_rows + taps_per_branch - 1) * nchan)",
               "taps": "oracle.synth_f32(taps_seed, taps_first, nchan * taps_per_branch)"}, open(GOLDEN + ".json", "w"), indent=1)
    np.save(GOLDEN + ".npy", golden_case(O)[1])
