"""The oversampled synthesis bank without a GPU: the restatement (tests/pfb_os_synth_ref.py: oracle.fft, oracle.fir) against
pfb_synth_ref at hop = nchan, against a float64 evaluation of the defining sum, and through a round trip with the oversampled
channelizer's restatement; the ref's stream model; both kernels (libredio_amd/csrc/pfb_os_synth_core.h) emulated thread by thread by a
stand-alone program that fences every index and compares with the ref bit for bit; the C ABI of the new symbols."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pfb_os_ref
import pfb_os_synth_ref as ref
import pfb_synth_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0533
BOUND = 2e-6  # relative L2 of a transform against float64
SHAPES = [(64, 4, 64), (64, 4, 32), (64, 4, 16), (64, 4, 48), (32, 3, 20), (12, 2, 5)]
HOPS = [1, 15, 16, 17, 63, 64, 65, 257, 529]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_nout_route_and_geometry_laws():
    assert [ref.nrows_per_hop(*s) for s in SHAPES] == [4, 8, 16, 6, 5, 5]
    assert [ref.nout(n, 64, 4, 32) for n in (0, 64 * 7 + 63, 64 * 8, 64 * 8 + 63, 64 * 9, 64 * 17 + 5)] == [0, 0, 32, 32, 64, 320]
    assert [ref.nout(n, 12, 2, 5) for n in (59, 60, 71, 72)] == [0, 5, 5, 10]
    assert all(ref.nout(n, M, P, M) == pfb_synth_ref.nout(n, M, P) for M, P in ((64, 16), (12, 3)) for n in range(0, 40 * M, 7))
    assert [ref.route(64, p, 32) for p in (4, 5, 8, 16, 32)] == [1, 0, 1, 1, 0]
    assert ref.route(64, 16, 16) == ref.route(64, 16, 64) == ref.route(32, 8, 16) == 0
    assert [ref.hops_per_wave(r) for r in (1, 64, 65, 2048 * 64, 2048 * 64 + 17, 2 ** 22)] == [64, 64, 64, 64, 80, 2048]
    assert [ref.waves(r) for r in (1, 64, 65, 257, 529, 2048 * 64, 2048 * 64 + 17)] == [1, 1, 2, 5, 9, 2048, 1639]
    # the oldest row drops out exactly for the residues whose offset in it would pass the window
    assert [ref.k0(j, 64, 4, 48) for j in (0, 15, 16, 47)] == [0, 0, 1, 1] and not any(ref.k0(j, 64, 4, 32) for j in range(32))
    assert [ref.k0(j, 12, 2, 5) for j in range(5)] == [0, 0, 0, 0, 1]
    # every tap is used by exactly one (k, j) of a hop's fold
    for M, P, H in SHAPES:
        L = ref.nrows_per_hop(M, P, H)
        used = sorted(ref.tap((L - 1 - k) * H + j, M, P) for j in range(H) for k in range(ref.k0(j, M, P, H), L))
        assert used == list(range(M * P))
    assert [ref.column(F, 0, 0, 64, 4, 32) for F in (0, 1, 2, 2 ** 64 - 530)] == [32, 0, 32, 32]


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("M,P", [(64, 16), (64, 4), (32, 8), (12, 3)])
def test_at_hop_nchan_the_ref_is_the_synthesizer(oracle, M, P, fused):
    X = oracle.synth_iq(SEED, M, (P + 20) * M + 5)
    h = oracle.synth_f32(3, P, M * P)
    want = pfb_synth_ref.synth(X, h, M, P, fused)
    for F in (0, 3):
        got = ref.synth(X, h, M, P, M, F, fused)
        assert got.shape == want.shape == (21 * M,) and np.array_equal(bits(got), bits(want))


def formula_f64(X, h, M, P, H, F):
    """y[n] = sum_r w_r[tau mod M] h[tap(tau - (F + r) H)] over the rows whose offset lies in [0, P M), w_r[c] = sum_k X_r[k] e^(+2 pi i k c / M)"""
    T = len(X) // M
    L = ref.nrows_per_hop(M, P, H)
    X = X[: T * M].astype(np.complex128).reshape(T, M)
    k = np.arange(M)
    W = X @ np.exp(2j * np.pi * ((k[:, None] * k[None, :]) % M) / M)
    h = h.astype(np.float64)
    y = np.zeros((T - L + 1) * H, np.complex128)
    for n in range(len(y)):
        tau = (F + L - 1) * H + n
        for r in range(T):
            o = tau - (F + r) * H
            if 0 <= o < P * M:
                y[n] += W[r, tau % M] * h[ref.tap(o, M, P)]
    return y


@pytest.mark.parametrize("F", [0, 1, 3])
@pytest.mark.parametrize("M,P,H", SHAPES)
def test_ref_against_the_float64_formula(oracle, M, P, H, F):
    hops = 9
    L = ref.nrows_per_hop(M, P, H)
    X = oracle.synth_iq(SEED, M + H, (hops + L - 1) * M + 3)
    h = oracle.synth_f32(3, P, M * P)
    got = ref.synth(X, h, M, P, H, F)
    assert got.shape == (hops * H,) == (ref.nout(len(X), M, P, H),)
    want = formula_f64(X, h, M, P, H, F)
    err = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    print(f"{M}x{P} hop {H} F={F}: relative L2 {err:.3e}")
    assert err <= BOUND


def windows(M, P, H):
    """an analysis and a synthesis prototype on window positions [0, M) with sum_r a[i - r H] g[i - r H] = 1: sin(pi (i + 1/2) / M) at
    H = M / 2, else the root of a ramp that rises over the M - H overlapped positions, stays at 1 and falls again (M / 2 <= H <= M)"""
    i = np.arange(M)
    if 2 * H == M:
        a = np.sin(np.pi * (i + 0.5) / M)
    else:
        ov = M - H
        assert 0 < ov <= H
        a = np.sqrt(np.where(i < ov, (i + 0.5) / ov, np.where(i < H, 1.0, 1.0 - (i - H + 0.5) / ov)))
    assert np.allclose(sum(np.pad(a * a, (r * H, 2 * M))[: 3 * M] for r in range(4))[M: 2 * M], 1.0)
    ha = np.zeros(M * P, np.float32)
    ha[:M] = a                                   # the channelizer's layout: tap n is window position n
    hs = np.zeros(M * P, np.float32)
    hs[[ref.tap(o, M, P) for o in range(M)]] = a  # h[tap(o)] = g[o]
    return ha, hs


@pytest.mark.parametrize("F", [0, 5])
@pytest.mark.parametrize("M,P,H", [(64, 4, 32), (64, 4, 48), (12, 2, 7)])
def test_round_trip_through_the_oversampled_channelizer(oracle, M, P, H, F):
    """channelize at hop H, synthesize at hop H: M x[(L - 1) H + n].  The bound is two transforms at the 8c bound each (4e-6); measured
    0.8e-7 to 1.1e-7 on the restatement in f32, a fortieth of it."""
    T = 40
    L = ref.nrows_per_hop(M, P, H)
    x = oracle.synth_iq(SEED, H, M * P + (T - 1) * H)
    ha, hs = windows(M, P, H)
    rows = pfb_os_ref.channelize(x, ha, M, P, H, F)
    assert rows.shape == (T, M)
    y = ref.synth(rows.reshape(-1), hs, M, P, H, F)
    assert len(y) == (T - L + 1) * H
    want = M * x[(L - 1) * H: (L - 1) * H + len(y)].astype(np.complex128)
    err = float(np.linalg.norm(y - want) / np.linalg.norm(want))
    print(f"round trip {M}x{P} hop {H} F={F}: relative L2 {err:.3e}")
    assert err <= 4e-6


@pytest.mark.parametrize("M,P,H", [(64, 4, 32), (64, 4, 48), (12, 2, 5)])
def test_stream_model_does_not_depend_on_the_split(oracle, M, P, H):
    L = ref.nrows_per_hop(M, P, H)
    n = (L + 36) * M + 3
    X = oracle.synth_iq(SEED, 7, n)
    h = oracle.synth_f32(3, 1, M * P)
    want = ref.synth(X, h, M, P, H)
    rng = np.random.default_rng(SEED + H)
    for cuts in ([n], [1] * 40 + [n - 40], [L * M - 1, 1, M - 1, 1, n - L * M - M], [0, 31, 0, 33, n - 64],
                 list(rng.multinomial(n, np.ones(9) / 9))):
        assert sum(cuts) == n
        s, got, at = ref.StreamModel(h, M, P, H), [], 0
        for c in cuts:
            assert s.nout(c) == ref.nout(s.pending + c, M, P, H)
            got.append(s.feed(X[at: at + c]))
            assert len(got[-1]) % H == 0 and s.pending < L * M
            at += c
        got = np.concatenate(got)
        assert np.array_equal(bits(got), bits(want)) and s.row == 37 and s.pending == n - s.row * M
    s.reset()
    assert s.pending == 0 and s.row == 0


def emu(*args, san=False):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_os_synth"), "-s"] + (["san"] if san else []))
    exe = os.path.join(ROOT, "tests", "_build", "emu_pfb_os_synth_san" if san else "emu_pfb_os_synth")
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (args, r.stderr)
    return int(r.stdout)


@functools.lru_cache(maxsize=None)
def wave_case(P, fused):
    """the longest input of the wave-kernel cases, its transformed rows and the outputs for both parities of F, computed once: every
    shorter case is a prefix (at hop 32 the column depends on F through its parity alone)"""
    import oracle
    X = oracle.synth_iq(SEED, P, 64 * (max(HOPS) + 2 * P - 1))
    h = oracle.synth_f32(3, 64 * P, 64 * P)
    W = ref.inverse_rows(X, 64)
    y = [ref.overlap_add(W, h, 64, P, 32, F, fused) for F in (0, 1)]
    for a in (X, h, W, *y):
        a.setflags(write=False)
    return X, h, y


def run_wave_cases(tmp_path, P, fused, cases, san=False):
    X, h, y = wave_case(P, fused)
    i, t, w = (str(tmp_path / n) for n in ("in.bin", "taps.bin", "want.bin"))
    h.tofile(t)
    for hpw, hops in cases:
        T = hops + 2 * P - 1
        X[: 64 * T].tofile(i)
        for F in (0, 1, 2 ** 64 - 1 - T):
            y[F & 1][: 32 * hops].tofile(w)
            assert emu("wave", P, int(fused), hpw, hops, F, i, t, w, san=san) == -(-hops // (hpw or ref.hops_per_wave(hops)))


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_wave_kernel_emulated_wavefront_by_wavefront(oracle, tmp_path, P, fused):
    """every lane of every wavefront, runs of 64 hops (the launcher's geometry at these sizes) and of 80 with a cut last wave whose
    tiles ask for rows past the end; F even, odd and 2^64 - 1 - T; the program fences every load, LDS index and store, wants every
    output written once, and compares with the ref bit for bit"""
    X, h, y = wave_case(P, fused)
    T = 65 + 2 * P - 1
    F = 2 ** 64 - 1 - T
    assert np.array_equal(bits(y[F & 1][: 32 * 65]), bits(ref.synth(X[: 64 * T], h, 64, P, 32, F, fused)))
    run_wave_cases(tmp_path, P, fused, [(0, n) for n in HOPS] + [(80, 170), (80, 161), (80, 80)])


OLA_CASES = [(64, 16, 16, 40, 0), (64, 5, 32, 40, 1), (64, 4, 48, 43, 0), (64, 4, 48, 43, 1), (32, 3, 20, 40, 9), (256, 4, 128, 9, 1), (12, 2, 5, 43, 0),
             (12, 2, 5, 43, 1), (100, 2, 100, 40, 0), (64, 4, 32, 529, 92)]  # M, P, H, hops, input rows per pass beyond L


@pytest.mark.parametrize("fused", [False, True])
def test_overlap_add_pass_emulated_thread_by_thread(oracle, tmp_path, fused):
    """route 0's second pass: the column, the taps and the store of every thread, in passes as the plan cuts them (L and L + 1 rows: one
    and two hops per pass)"""
    i, t, w = (str(tmp_path / n) for n in ("w.bin", "taps.bin", "want.bin"))
    for M, P, H, hops, extra in OLA_CASES:
        L = ref.nrows_per_hop(M, P, H)
        X = oracle.synth_iq(SEED, M, (hops + L - 1) * M)
        h = oracle.synth_f32(3, M, M * P)
        W = ref.inverse_rows(X, M)
        W.tofile(i)
        h.tofile(t)
        for F in (0, 3, 2 ** 64 - hops - L):
            ref.overlap_add(W, h, M, P, H, F, fused).tofile(w)
            assert emu("ola", M, P, H, int(fused), hops, F, L + extra, i, t, w) == -(-hops // (extra + 1))


def test_emulation_under_sanitizers(oracle, tmp_path):
    """the same program built with -fsanitize=address,undefined and run directly: a plain host program, nothing to preload"""
    run_wave_cases(tmp_path, 8, True, [(0, 17), (0, 65)], san=True)
    run_wave_cases(tmp_path, 16, False, [(80, 161)], san=True)
    M, P, H, hops = 12, 2, 5, 43
    L = ref.nrows_per_hop(M, P, H)
    X, h = oracle.synth_iq(SEED, M, (hops + L - 1) * M), oracle.synth_f32(3, M, M * P)
    W = ref.inverse_rows(X, M)
    i, t, w = (str(tmp_path / n) for n in ("bw.bin", "btaps.bin", "bwant.bin"))
    W.tofile(i)
    h.tofile(t)
    ref.overlap_add(W, h, M, P, H, 3, True).tofile(w)
    assert emu("ola", M, P, H, 1, hops, 3, L + 4, i, t, w, san=True) == 9


def test_emulation_rejects_wrong_output(oracle, tmp_path):
    """the program's comparison is live: the samples for the other parity of F fail it"""
    X, h, y = wave_case(4, False)
    i, t, w = (str(tmp_path / n) for n in ("in.bin", "taps.bin", "want.bin"))
    X[: 64 * (17 + 7)].tofile(i)
    h.tofile(t)
    y[1][: 32 * 17].tofile(w)
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_os_synth"), "-s"])
    r = subprocess.run([os.path.join(ROOT, "tests", "_build", "emu_pfb_os_synth"), "wave", "4", "0", "0", "17", "0", i, t, w], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 2 and "same_bits" in r.stderr


NAMES = ["redio_pfb_os_synth_" + n for n in ("create", "destroy", "nout", "hop", "route", "is_fused", "set_unfused", "set_chunk_rows", "reserve", "enqueue")] + [
    f"redio_pfb_os_synth_stream_{s}" for s in ("create", "destroy", "reset", "nout", "pending", "enqueue")]


def test_header_and_exports(redio):
    L = C.CDLL(redio.LIBREDIO)
    assert '#include "redio_pfb_os_synth.h"' in open(os.path.join(ROOT, "include", "redio.h")).read()
    hdr = open(os.path.join(ROOT, "include", "redio_pfb_os_synth.h")).read()
    assert "typedef struct redio_pfb_os_synth redio_pfb_os_synth;" in hdr and "typedef struct redio_pfb_os_synth_stream redio_pfb_os_synth_stream;" in hdr
    declared = set(re.findall(r"\b(redio_pfb_os_synth\w*)\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(NAMES)
    for n in sorted(declared):
        assert hasattr(L, n), f"libredio.so does not export {n}"
    assert hasattr(redio, "OversampledSynthesizer") and issubclass(redio.OversampledSynthesizerStream, redio.Stream)
