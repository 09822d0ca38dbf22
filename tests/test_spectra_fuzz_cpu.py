"""The generator of tests/fuzz_spectra.py, and the five restatements it compares the device with, checked without a GPU.

Generator coverage: the dry mode (`fuzz_spectra.py --draw 6000 SEED`, the seed of tests/test_gpu_fuzz_spectra.py) is run as the
command it is, in a process that must import neither torch nor the product library, and every route combination the driver of
pspec_api.hip (the polyphase spectrometer's entries included), the stream layer and the real-input plans distinguish has to turn up
in at least 1 % of the cases; the polyphase spectrometer's workgroup kernel (route 2: the plan's one_kernel flag) per channel count,
split mode, entry and alignment among them.  Route 2 is in the opening round of the GPU test's own runs, and the tool's restated launch
geometry is pfb_pspec_p2_core.h's.

Restatements against float64: the counterpart of test_oracle_random.py for fftr_ref, ovsave_real_ref, pspec_ref, pspec_real_ref and
pfb_pspec_ref, on the generator's own first 400 shapes (the opening round of all eight families and as many again), unspiced.  The
bounds are the project's: 2e-6 for transforms and spectra (test_pspec_cpu.py, test_fftr_cpu.py) and
2e-6 sum|taps| sqrt(log2 N) + 1e-7 for overlap-save (test_ovsave_real_cpu.py), each times max(1, p / 8) with p the largest prime
factor of the complex transform's size, the rule of test_oracle_random.py.  The polyphase spectrometer (exact: the float64 branch fold,
numpy's transform across the branches, |.|^2 summed over K rows) is held to the spectra rule with p of M as it stands: its measured
worst is under half of it, so the taps ask for no factor of their own.
Worst distances over those 400 cases, as values and as fractions of their bounds (measure: max|got - exact| / max(exact) for the
spectra, relative L2 for the transforms, the largest absolute error for overlap-save):
    pspec        3.6e-07, 0.18 of its bound        pspec_real   3.8e-07, 0.19
    pspec_u8     4.2e-07, 0.21                     fftr         1.5e-07, 0.07
    ovsave_real  8.5e-08, 0.08                     streams      3.0e-07, 0.15
    pfb_pspec    2.7e-07, 0.13                     pfb_streams  2.7e-07, 0.14
(the polyphase shapes are mostly workgroup-kernel ones now; before that: pfb_pspec 2.8e-07, 0.14, pfb_streams 2.3e-07, 0.11)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fftr_ref
import fuzz_spectra as fz
import ovsave_real_ref
import pfb_pspec_ref
import pspec_real_ref
import pspec_ref

SEED = 11          # tests/test_gpu_fuzz_spectra.py runs the tool with this seed
DRAWN, LEAST = 6000, 60
CHECKED = 400      # cases of the float64 check: the opening round of every family and as many again at random
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_spectra.py")
# the dry mode as a command, in an interpreter that afterwards reports whether torch or the product library were imported
DRY = ("import runpy, sys\n"
       "sys.argv = [sys.argv[1]] + sys.argv[2:]\n"
       "try:\n    runpy.run_path(sys.argv[0], run_name='__main__')\nexcept SystemExit as e:\n    assert not e.code, e.code\n"
       "sys.exit(3 if 'torch' in sys.modules or 'libredio_amd' in sys.modules else 0)\n")


@pytest.fixture(scope="module")
def drawn():
    out = subprocess.run([sys.executable, "-c", DRY, TOOL, "--draw", str(DRAWN), str(SEED)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    cases = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(cases) == DRAWN
    return cases


def plan_key(c):
    return json.dumps({k: c[k] for k in ("family", "N", "inverse", "ntaps", "taps", "tseed", "K", "step", "window", "wseed", "M", "P", "fir_fused", "block") if k in c}, sort_keys=True)


def test_the_dry_mode_draws_what_a_run_draws(drawn):
    """the same cases from the generator in this process: an opening round of every family first, then families at random"""
    gen = fz.Gen(SEED)
    again = [gen.draw(f) for _, f in zip(range(DRAWN), fz.sequence(gen, None))]
    assert json.loads(json.dumps(again)) == drawn
    opening = [c["family"] for c in drawn[: fz.OPENING * len(fz.FAMILIES)]]
    assert opening == [f for f in fz.FAMILIES for _ in range(fz.OPENING)]


def test_every_route_combination_is_drawn_often_enough(drawn):
    by = {f: [c for c in drawn if c["family"] == f] for f in fz.FAMILIES}
    r = lambda c: c["route"]
    cond = {}
    for f in fz.FAMILIES:
        cond[f"{f} present"] = by[f]
    for f in ("fftr", "ovsave_real", "pspec", "pspec_u8", "pspec_real"):
        cond[f"{f} fused"] = [c for c in by[f] if r(c)["fused"]]
        cond[f"{f} generic"] = [c for c in by[f] if not r(c)["fused"]]
    for f in ("pspec", "pspec_u8", "pspec_real"):
        cond[f"{f} packs"] = [c for c in by[f] if r(c)["packs"]]
        cond[f"{f} does not pack"] = [c for c in by[f] if not r(c)["packs"]]
        cond[f"{f} K <= 16"] = [c for c in by[f] if c["K"] <= 16]
        for mode in (1, 2):
            cond[f"{f} K > 16 in mode {mode}"] = [c for c in by[f] if c["K"] > 16 and r(c)["segments2"] and c["mode"] == mode]
        cond[f"{f} step > N"] = [c for c in by[f] if c["step"] > c["N"] and r(c)["H>W"]]
        cond[f"{f} stream with H > W"] = [c for c in by["streams"] if c["kind"] == f and r(c)["H>W"]]
    cond["pspec_real odd step"] = [c for c in by["pspec_real"] if r(c)["odd_step"]]
    cond["pspec_real 4-byte base"] = [c for c in by["pspec_real"] if r(c)["base"] == 4]
    cond["pspec_u8 at 2048 or 4096"] = [c for c in by["pspec_u8"] if r(c)["fft_u8"] in (2048, 4096)]
    cond["pspec_u8 base not a multiple of 8"] = [c for c in by["pspec_u8"] if r(c)["base"] % 8]
    cond["ovsave_real even ntaps"] = [c for c in by["ovsave_real"] if r(c)["ntaps_even"]]
    cond["fftr strided forward with overlap"] = [c for c in by["fftr"] if r(c)["strided"] and not c["inverse"] and r(c)["overlap"] and c["in_stride"] < c["N"]]
    cond["refusal expected"] = [c for c in drawn if r(c).get("refusal")]
    # the polyphase spectrometer: a pfb_pspec case runs the cf32 entry, from_bytes and the composition; "from bytes" alone is a u8 stream
    pfb, pst8 = by["pfb_pspec"], [c for c in by["pfb_streams"] if c["u8"]]
    for name in ("fused", "one_kernel", "two_pass"):
        cond[f"pfb_pspec {name}"] = [c for c in pfb if r(c)[name]]
        cond[f"pfb_streams {name} from bytes"] = [c for c in pst8 if r(c)[name]]
    cond["pfb_pspec m64_generic"] = [c for c in pfb if r(c)["m64_generic"]]
    cond["pfb_pspec K <= 16"] = [c for c in pfb if c["K"] <= 16]
    for mode in (1, 2):
        cond[f"pfb_pspec fused K > 16 in mode {mode}"] = [c for c in pfb if r(c)["fused"] and c["K"] > 16 and r(c)["segments2"] and c["mode"] == mode]
    cond["pfb_pspec fir_fused"] = [c for c in pfb if r(c)["fir_fused"]]
    cond["pfb_pspec not fir_fused"] = [c for c in pfb if not r(c)["fir_fused"]]
    cond["pfb_pspec rows == 0"] = [c for c in pfb if c["rows"] == 0]
    cond["pfb_pspec K == 1"] = [c for c in pfb if c["K"] == 1]
    cond["pfb_pspec base not a multiple of 8"] = [c for c in pfb if r(c)["base"] % 8]
    cond["pfb_pspec cbase == 8"] = [c for c in pfb if r(c)["cbase"] == 8]
    cond["pfb_pspec fused, more than two wavefronts"] = [c for c in pfb if r(c)["fused"] and c["rows"] > 2 * -(-64 // c["K"])]
    for u8 in (False, True):
        for name in ("zero_piece", "short_piece", "long_piece", "odd_piece", "reset"):
            cond[f"pfb_streams u8={u8} {name}"] = [c for c in by["pfb_streams"] if c["u8"] == u8 and r(c)[name]]
    # the workgroup kernel (route 2): the plan's flag on a one-kernel shape of the inner channelizer
    both = pfb + by["pfb_streams"]
    for c in both:
        assert r(c)["route"] == (1 if r(c)["fused"] else 2 if c["block"] and r(c)["one_kernel"] else 0), c
    two, two_st = [c for c in pfb if r(c)["route"] == 2], [c for c in by["pfb_streams"] if r(c)["route"] == 2]
    for M in fz.PFB_ONE_KERNEL:
        cond[f"route 2 at {M} channels"] = [c for c in two + two_st if c["M"] == M]
    for mode in (0, 1, 2):
        cond[f"pfb_pspec route 2 in mode {mode}"] = [c for c in two if c["mode"] == mode]
        for big in (False, True):   # a set test: every mode either side of K = 16, in a launch of more than one workgroup
            assert any(c["mode"] == mode and (c["K"] > fz.SEG) == big and r(c)["geometry"]["groups"] > 1 for c in two), (mode, big)
    cond["pfb_pspec route 2 with K > 16"] = [c for c in two if c["K"] > fz.SEG]
    cond["pfb_pspec route 2 by segments"] = [c for c in two if r(c)["split"]]
    cond["pfb_pspec route 2 from bytes at an odd 2-byte base"] = [c for c in two if c["base"] % 4 == 2]
    cond["pfb_pspec route 2 with cf32 base 8"] = [c for c in two if c["cbase"] == 8]
    cond["route 2 spiced"] = [c for c in two + two_st if c["spice"]]
    cond["pfb_pspec route 2 in more than one workgroup"] = [c for c in two if r(c)["geometry"]["groups"] > 1]
    cond["pfb_pspec route 2 with a short last stream"] = [c for c in two if r(c)["geometry"]["units"] % r(c)["geometry"]["ups"]]
    cond["pfb_streams on route 2 from cf32"] = [c for c in two_st if not c["u8"]]
    cond["pfb_streams on route 2 from u8"] = [c for c in two_st if c["u8"]]
    cond["the flag on a shape with no block form"] = [c for c in both if r(c)["flag_no_form"]]
    cond["a one-kernel shape without the flag, down the generic route"] = [c for c in both if r(c)["one_kernel"] and r(c)["route"] == 0]
    seen, again = {}, []
    for c in drawn:
        if c["family"] not in ("streams", "pfb_streams"):
            k = plan_key(c)
            if any(rows != c["rows"] for rows in seen.get(k, ())):
                again.append(c)
            seen.setdefault(k, set()).add(c["rows"])
    cond["a plan shape again with another row count"] = again
    # the streams' cuts: a zero-length piece, one shorter than a window, one longer than two, odd lengths, an end inside a skipped gap
    pst = [c for c in by["streams"] if c["kind"] != "ovsave_real"]
    for name in ("zero_piece", "short_piece", "long_piece", "odd_piece", "ends_in_gap", "reset"):
        cond[f"streams {name}"] = [c for c in by["streams"] if r(c)[name]]
    counts = {k: len(v) for k, v in cond.items()}
    print(counts)
    short = {k: n for k, n in counts.items() if n < LEAST}
    assert not short, short
    assert 4 * len([c for c in pst if r(c)["H>W"]]) >= len(pst)       # a quarter of the power-spectrum streams skip
    assert 2 * len(cond["streams reset"]) >= 0.8 * len(by["streams"])  # about half reset and run again
    sizes = {r(c)["staging"] for c in drawn if r(c).get("staging")}
    assert sizes >= {65536, 8194, 16388, 131072}, sizes
    # every case respects the bound that keeps the restatement fast, the large sizes' one or two transforms excepted
    for c in drawn:
        real = c["family"] in ("pspec_real", "fftr", "ovsave_real") or c.get("kind") in ("pspec_real", "ovsave_real")
        ntr = {"fftr": c["rows"], "ovsave_real": 2 * c["rows"]}.get(c["family"], c["rows"] * c.get("K", 1))
        if c["family"] in ("streams", "pfb_streams"):
            continue
        if c["family"] == "pfb_pspec":
            assert c["rows"] * c["K"] <= fz.transforms_allowed(c["M"]) and c["rows"] * c["K"] * c["M"] <= fz.POINTS, c
        elif r(c).get("staging"):
            assert ntr <= 2, c
        else:
            assert ntr * (c["N"] // 2 if real else c["N"]) <= fz.POINTS, c


def test_route_2_is_in_the_opening_rounds_of_the_gpu_runs():
    """tests/test_gpu_fuzz_spectra.py runs the tool per family (--only) at SEED: the OPENING cases it runs whatever the machine's speed
    hold the workgroup kernel"""
    for fam in ("pfb_pspec", "pfb_streams"):
        gen = fz.Gen(SEED)
        opening = [gen.draw(f) for _, f in zip(range(fz.OPENING), fz.sequence(gen, fam))]
        assert any(c["route"]["route"] == 2 for c in opening), fam


def test_the_tools_block_geometry_is_the_headers(drawn):
    """pfb_block_consts and pfb_block_geometry against libredio_amd/csrc/pfb_pspec_p2_core.h as tests/emu_pfb_pspec_p2 compiles it, on
    the drawn route-2 cases and on devices of 1 to 304 CUs: streams per workgroup, rows per iteration, auto mode's threshold, the units
    per stream, and the workgroup count -- the last stream of the last workgroup that owns a unit, the first slot behind the grid owns
    none; the case's own record is the one for NOMINAL_CUS"""
    import ctypes as C
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_pspec_p2"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pfb_pspec_p2.so"))
    L = C.c_long
    E.emu_pfbspec_p2_units_per_stream.argtypes, E.emu_pfbspec_p2_units_per_stream.restype = [L, L, C.c_int, L, C.c_int], L
    E.emu_pfbspec_p2_split_rows.argtypes, E.emu_pfbspec_p2_split_rows.restype = [L, L, C.c_int], L
    E.emu_pfbspec_p2_stream.argtypes, E.emu_pfbspec_p2_stream.restype = [L, L, L, L, L, C.c_int, C.POINTER(L)], None
    two = [c for c in drawn if c["family"] == "pfb_pspec" and c["route"]["route"] == 2]
    assert len(two) >= 3 * LEAST
    for c in two:
        M, K, rows, mode = c["M"], c["K"], c["rows"], c["mode"]
        assert c["route"]["geometry"] == fz.pfb_block_geometry(M, K, rows, mode, fz.NOMINAL_CUS) and c["route"]["split"] == c["route"]["geometry"]["split"], c
        for cus in (1, 2, 8, 256, 304):
            g = fz.pfb_block_geometry(M, K, rows, mode, cus)
            assert (g["G"], g["TR"]) == (E.emu_pfbspec_p2_streams_per_group(M), E.emu_pfbspec_p2_rows_per_iter(M)), c
            want_split = K > fz.SEG and (mode == 2 or (mode == 0 and rows < E.emu_pfbspec_p2_split_rows(K, cus, M)))
            assert g["split"] == want_split and g["units"] == rows * (-(-K // fz.SEG) if want_split else 1), (c, cus)
            if not rows:
                continue
            assert g["ups"] == E.emu_pfbspec_p2_units_per_stream(g["units"], K, int(g["split"]), cus, M), (c, cus)
            st = (L * 4)()
            E.emu_pfbspec_p2_stream(g["streams"] - 1, g["ups"], g["units"], rows * K, K, int(g["split"]), st)
            assert st[0] < st[1] == g["units"] and st[3] == rows * K, (c, cus, list(st))
            E.emu_pfbspec_p2_stream(g["streams"], g["ups"], g["units"], rows * K, K, int(g["split"]), st)
            assert st[0] == st[1] == g["units"] and g["groups"] == -(-g["streams"] // g["G"]), (c, cus, list(st))


def exact_rows(x, N, K, step, window, real):
    """float64: the sum over K transforms of |fft|^2 (|rfft|^2) of the windowed rows"""
    nt = pspec_ref.nrows(len(x), N, K, step) * K
    rows = np.stack([x[t * step: t * step + N] for t in range(nt)]).astype(np.float64 if real else np.complex128)
    if window is not None:
        rows = rows * window.astype(np.float64)
    P = np.abs(np.fft.rfft(rows, axis=1) if real else np.fft.fft(rows, axis=1)) ** 2
    return P.reshape(-1, K, P.shape[1]).sum(axis=1)


def exact_pfb_rows(x, h, M, P, K):
    """float64: the branch fold y[t][m] = sum_p x[(t + p) M + m] h[p M + m], numpy's transform across the branches (the convention of
    test_channelizer_against_its_polyphase_definition), |.|^2 summed over K rows"""
    nt = pfb_pspec_ref.nrows(len(x), M, P, K) * K
    X = x[: M * (P - 1 + nt)].astype(np.complex128).reshape(P - 1 + nt, M)
    H = h.astype(np.float64).reshape(P, M)
    branch = np.stack([(X[t:t + P] * H).sum(axis=0) for t in range(nt)])
    return (np.abs(np.fft.fft(branch, axis=1)) ** 2).reshape(-1, K, M).sum(axis=1)


def test_restatements_against_float64_on_the_generators_shapes(oracle):
    gen = fz.Gen(SEED)
    worst = {}

    def note(fam, err, tol, c):
        w = worst.setdefault(fam, [0.0, 0.0])
        if err / tol > w[0]:
            w[:] = [err / tol, err]
        assert err <= tol, (fam, err, tol, c)

    for _, fam in zip(range(CHECKED), fz.sequence(gen, None)):
        c = gen.draw(fam)
        kind = c.get("kind", fam)
        if fam in ("pfb_pspec", "pfb_streams"):
            M, P, K = c["M"], c["P"], c["K"]
            h = fz.pfb_taps_of(oracle, c)
            for u8 in ((False, True) if fam == "pfb_pspec" else (c["u8"],)):
                x = fz.pfb_input(oracle, c, u8, spiced=False)
                xs = fz.samples_of(oracle, x) if u8 else x
                got = pfb_pspec_ref.spectrum(xs, h, M, P, K, c["fir_fused"])
                if len(got):
                    want = exact_pfb_rows(xs, h, M, P, K)
                    assert got.shape == want.shape
                    note(fam, float(np.abs(got - want).max() / want.max()), 2e-6 * max(1.0, fz.largest_prime_factor(M) / 8.0), c)
            continue
        x = fz.case_input(oracle, c, spiced=False)
        N = c["N"]
        rough = max(1.0, fz.largest_prime_factor(max(N if kind in ("pspec", "pspec_u8") else N // 2, 1)) / 8.0)
        if kind == "fftr":
            nin = N // 2 + 1 if c["inverse"] else N
            rows = np.stack([x[b * c["in_stride"]: b * c["in_stride"] + nin] for b in range(c["rows"])])
            if c["inverse"]:
                got, want = fftr_ref.fftri_rows(rows, N), np.fft.irfft(rows.astype(np.complex128), n=N, axis=1) * N
            else:
                got, want = fftr_ref.fftr_rows(rows, N), np.fft.rfft(rows.astype(np.float64), axis=1)
            note(fam, np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30), 2e-6 * rough, c)
        elif kind == "ovsave_real":
            taps = fz.taps_of(oracle, c)
            got = ovsave_real_ref.overlap_save_real(x, taps, N)
            if len(got):
                want = np.correlate(x.astype(np.float64), taps.astype(np.float64), "valid")[: len(got)]
                tol = (2e-6 * float(np.abs(taps).sum()) * np.sqrt(np.log2(N)) + 1e-7) * rough
                note(fam, float(np.abs(got - want).max()), tol, c)
        else:
            real = kind == "pspec_real"
            xs = fz.samples_of(oracle, x) if kind == "pspec_u8" else x
            w = fz.window_of(oracle, c)
            got = (pspec_real_ref if real else pspec_ref).power_spectrum(xs, N, c["K"], c["step"], w)
            if len(got):
                want = exact_rows(xs, N, c["K"], c["step"], w, real)
                assert got.shape == want.shape
                note(fam, float(np.abs(got - want).max() / want.max()), 2e-6 * rough, c)
    for fam, (frac, err) in sorted(worst.items()):
        print(f"{fam:12s} worst distance {err:.2e}, {frac:.2f} of its bound")
    assert set(worst) == set(fz.FAMILIES)
