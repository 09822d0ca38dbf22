"""The generator of tests/fuzz_banks.py, and the three restatements it compares the device with, checked without a GPU.

Generator coverage: the dry mode (`fuzz_banks.py --draw 6000 SEED`, the seed of tests/test_gpu_fuzz_banks.py) is run as the command it
is, in a process that must import neither torch nor the product library, and every branch and shape edge the one driver of
pfb_bank.hip, the cut of pfb_bank_cut.h, the three wave kernels, the oversampled channelizer's workgroup kernel (route 2: the plan's
one_kernel flag) and the stream layer distinguish has to turn up in at least 1 % of the cases; the staging size 8194 has to turn up for
each one-call family, the flag on 1024 x 16 (no workgroup form) too.  Route 2 is in the opening round of the GPU test's own runs, and
the tool's restated launch geometry is pfb_os_p2_core.h's.

Restatements against float64: the counterpart of test_oracle_random.py for pfb_synth_ref, pfb_os_ref and pfb_os_synth_ref (and their
stream models), on the generator's own first CHECKED unspiced cases whose output has 1 to 4096 values, and behind them the first
such case at 512 and at 1024 channels if those have not met one.  The exact values are the defining
sums of test_pfb_synth_cpu.py, test_pfb_os_cpu.py and test_pfb_os_synth_cpu.py, vectorised, in float64.  The bound is the project's:
relative L2 of 2e-6 times max(1, p / 8) with p the largest prime factor of M, the rule of test_oracle_random.py, with no
factor for the fold length: the distance grows like the square root of the fold (about 2e-8 sqrt(L) for the overlap-add over L rows), and
the longest fold the generator can draw (L = 20 M with (L + 1) M <= 2^18: some 2300 rows) stays at half of the rule; measured apart
from this test at H = 1: 7.8e-07 at (100, 20), L = 2000, and 8.6e-07 at (96, 20), L = 1920.
Worst relative L2 distances over those cases, as values and as fractions of their bounds:
    pfb_synth     1.2e-07, 0.06 of its bound, at (M, P, H) = (210, 2, 210)
    pfb_os        1.3e-07, 0.06, at (256, 16, 128): a shape of the workgroup kernel
    pfb_os_synth  7.6e-07, 0.38, at (64, 16, 1): a fold of L = 1024 rows
    bank_streams  1.3e-07, 0.06, at (100, 18, 99)
(before the generator drew the workgroup kernel's shapes: 1.2e-07 at (48, 11, 48), 1.3e-07 at (100, 16, 41), 1.1e-06, 0.52 of the bound, at
(64, 16, 1), and 1.1e-07 at (7, 2, 7)).  At 512 and 1024 channels, over the cases of this check: 1.2e-07, 0.06, at pfb_os (512, 8, 256) and
1.2e-07, 0.06, at pfb_os (1024, 8, 512); measured apart from this test over every such case of the 6000 (a 25 s run): 2.0e-07, 0.10 of
the bound, at pfb_os_synth (512, 8, 44) and at pfb_os_synth (1024, 4, 54).  The restatements alone stay far inside the rule there."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import fuzz_banks as fz
import fuzz_spectra as fs
import pfb_os_p2_ref as p2

SEED = 11          # tests/test_gpu_fuzz_banks.py runs the tool with this seed
DRAWN, LEAST = 6000, 60
CHECKED = 240      # cases of the float64 check
MOST_VALUES = 4096
TOOL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fuzz_banks.py")
# the dry mode as a command, in an interpreter that afterwards reports whether torch or the product library were imported
DRY = ("import runpy, sys\n"
       "sys.argv = [sys.argv[1]] + sys.argv[2:]\n"
       "try:\n    runpy.run_path(sys.argv[0], run_name='__main__')\nexcept SystemExit as e:\n    assert not e.code, e.code\n"
       "sys.exit(3 if 'torch' in sys.modules or 'libredio_amd' in sys.modules else 0)\n")
ONE_CALL = fz.FAMILIES[:3]


@pytest.fixture(scope="module")
def drawn():
    out = subprocess.run([sys.executable, "-c", DRY, TOOL, "--draw", str(DRAWN), str(SEED)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    cases = [json.loads(line) for line in out.stdout.splitlines()]
    assert len(cases) == DRAWN
    return cases


def plan_key(c):
    return json.dumps({k: c[k] for k in ("kind", "M", "P", "H", "fused", "taps", "tseed", "block")}, sort_keys=True)


def test_the_dry_mode_draws_what_a_run_draws(drawn):
    """the same cases from the generator in this process: an opening round of every family first, then families at random"""
    gen = fz.Gen(SEED)
    again = [gen.draw(f) for _, f in zip(range(DRAWN), fz.sequence(gen, None))]
    assert json.loads(json.dumps(again)) == drawn
    opening = [c["family"] for c in drawn[: fz.OPENING * len(fz.FAMILIES)]]
    assert opening == [f for f in fz.FAMILIES for _ in range(fz.OPENING)]
    # FUZZ_TRACE / FUZZ_STATE: the state written before case 150, through JSON, draws case 150 and the ones behind it again
    gen = fz.Gen(SEED)
    for k in range(150):
        gen.draw("bank_streams" if k % 2 else "pfb_os_synth")
    st = json.loads(json.dumps(gen.state()))
    want = [gen.draw(f) for f in ("pfb_os", "bank_streams", "pfb_synth")]
    back = fz.Gen(1)
    back.restore(st)
    assert [back.draw(f) for f in ("pfb_os", "bank_streams", "pfb_synth")] == want
    only = fz.Gen(SEED)
    assert all(only.draw(f)["family"] == "pfb_os" for _, f in zip(range(40), fz.sequence(only, "pfb_os")))


def test_every_branch_and_shape_edge_is_drawn_often_enough(drawn):
    by = {f: [c for c in drawn if c["family"] == f] for f in fz.FAMILIES}
    calls = [c for c in drawn if c["family"] in ONE_CALL]
    r = lambda c: c["route"]
    cond = {}
    for f in fz.FAMILIES:
        cond[f"{f} present"] = by[f]
    for f in ONE_CALL:
        cond[f"{f} wave route"] = [c for c in by[f] if r(c)["route"] == 1]
        cond[f"{f} two-pass shape"] = [c for c in by[f] if r(c)["two_pass_shape"]]
        cond[f"{f} M == 64 without the wave route"] = [c for c in by[f] if r(c)["m64_generic"]]
    route0 = [c for c in calls if r(c)["route"] == 0 and c["units"] and not c["refusal"]]
    cond["a wave shape sent down route 0"] = [c for c in route0 if r(c)["wave_shape"]]
    cond["the default chunk"] = [c for c in route0 if c["chunk"] == 0]
    cond["the chunk at min_rows"] = [c for c in route0 if c["chunk"] == r(c)["min_rows"]]
    cond["a chunk below min_rows, which counts as min_rows"] = [c for c in route0 if 0 < c["chunk"] < r(c)["min_rows"]]
    cond["three or more passes with a short last one"] = [c for c in route0 if r(c)["passes"] >= 3 and r(c)["short_last"]]
    cond["one pass"] = [c for c in route0 if r(c)["passes"] == 1]
    cond["units == 0"] = [c for c in calls if c["units"] == 0]
    cond["units == 1"] = [c for c in calls if c["units"] == 1]
    cond["more than two wavefronts on the wave route"] = [c for c in calls if r(c)["route"] == 1 and c["units"] > 128]
    cond["an odd unit count on the wave route"] = [c for c in calls if r(c)["route"] == 1 and c["units"] % 2]
    rowed = [c for c in calls if c["family"] != "pfb_synth"]
    cond["first_row odd"] = [c for c in rowed if c["first_row"] % 2]
    cond["first_row at or above 2^32"] = [c for c in rowed if c["first_row"] >= 1 << 32]
    cond["first_row at the top"] = [c for c in rowed if c["first_row"] == fz.TOP - (c["units"] if c["family"] == "pfb_os" else c["units"] + r(c)["min_rows"] - 1)]
    cond["input base 8"] = [c for c in calls if c["in_base"] == 8]
    cond["output base 8"] = [c for c in calls if c["out_base"] == 8]
    cond["fused"] = [c for c in drawn if c["fused"]]
    cond["not fused"] = [c for c in drawn if not c["fused"]]
    over = [c for c in drawn if c["kind"] != "pfb_synth"]
    cond["H == M"] = [c for c in over if c["H"] == c["M"]]
    cond["H == 1"] = [c for c in over if c["H"] == 1]
    cond["gcd(M, H) == 1 with H > 1"] = [c for c in over if c["H"] > 1 and math.gcd(c["M"], c["H"]) == 1]
    cond["M / 2 < H < M"] = [c for c in over if c["M"] < 2 * c["H"] < 2 * c["M"]]
    cond["P == 1"] = [c for c in drawn if c["P"] == 1]
    cond["M not a power of two"] = [c for c in drawn if c["M"] & (c["M"] - 1)]
    cond["M prime"] = [c for c in drawn if fz.is_prime(c["M"])]
    cond["synthesis with L H > P M"] = [c for c in drawn if r(c)["skips_oldest"]]
    for c in cond["synthesis with L H > P M"]:
        assert c["kind"] == "pfb_os_synth" and fz.nrows_per_hop(c["M"], c["P"], c["H"]) * c["H"] > c["P"] * c["M"]
    cond["a trailing partial"] = [c for c in calls if c["units"] and c["n"] > (c["units"] - 1) * fz.cut_of(c["kind"], c["M"], c["P"], c["H"])[1] + fz.cut_of(c["kind"], c["M"], c["P"], c["H"])[0]]
    cond["reserve called first"] = [c for c in drawn if c["reserve"]]
    cond["spiced"] = [c for c in drawn if c["spice"]]
    cond["refusal expected"] = [c for c in calls if c["refusal"]]
    seen, again = {}, []
    for c in calls:
        k, now = plan_key(c), (r(c)["route"], c["chunk"], c["units"])
        if any(was != now for was in seen.get(k, ())):
            again.append(c)
        seen.setdefault(k, set()).add(now)
    cond["a plan shape again with another route, chunk or length"] = again
    for kind in fz.STREAM_KINDS:
        for name in ("zero_piece", "short_piece", "long_piece", "odd_piece", "reset"):
            cond[f"bank_streams {kind} {name}"] = [c for c in by["bank_streams"] if c["kind"] == kind and r(c)[name]]
        for unfused in (False, True):   # the plan behind a stream on both routes: a set test per class, 1 % over the three
            assert any(r(c)["wave_shape"] and c["unfused"] == unfused for c in by["bank_streams"] if c["kind"] == kind), (kind, unfused)
    cond["bank_streams on a wave shape sent down route 0"] = [c for c in by["bank_streams"] if c["unfused"]]
    cond["bank_streams on the wave route"] = [c for c in by["bank_streams"] if r(c)["route"] == 1]
    # the oversampled channelizer's workgroup kernel: route 2, from the plan's flag on a shape that has the form
    two = [c for c in by["pfb_os"] if r(c)["route"] == 2]
    for c in two:
        assert c["block"] and not c["unfused"] and p2.route(c["M"], c["P"], c["H"], True) == 2, c
    for c in drawn:   # the tool's rule is the one the kernel's own tests use
        if c["kind"] == "pfb_os":
            assert r(c)["route"] == (0 if c["unfused"] else p2.route(c["M"], c["P"], c["H"], c["block"])), c
        else:
            assert not c["block"] and r(c)["route"] < 2, c
    GT = {c["M"]: fz.block_consts(c["M"]) for c in two}
    for M in fz.BLOCK_M:
        cond[f"route 2 at {M} channels"] = [c for c in two if c["M"] == M]
    cond["route 2, 512 or 1024 channels, input base 8 (the 8-byte load form)"] = [c for c in two if c["M"] >= 512 and c["in_base"] == 8]
    cond["route 2, 512 or 1024 channels, input base 0 (the pair form)"] = [c for c in two if c["M"] >= 512 and c["in_base"] == 0]
    cond["route 2 with output base 8"] = [c for c in two if c["out_base"] == 8]
    cond["route 2 with first_row odd"] = [c for c in two if c["first_row"] % 2]
    cond["route 2 with first_row even"] = [c for c in two if not c["first_row"] % 2]
    cond["route 2 with more than 64 G rows"] = [c for c in two if c["units"] > 64 * GT[c["M"]][0]]
    cond["route 2 with a row count that is no multiple of TR"] = [c for c in two if c["units"] % GT[c["M"]][1]]
    cond["route 2 with no row or one row"] = [c for c in two if c["units"] <= 1]
    assert {0, 1} <= {c["units"] for c in two}
    cond["route 2 spiced"] = [c for c in two if c["spice"] and not c["refusal"]]
    cond["route 2 not fused"] = [c for c in two if not c["fused"]]
    cond["route 2 with a refusal expected"] = [c for c in two if c["refusal"]]
    cond["a block shape sent down route 0"] = [c for c in by["pfb_os"] if r(c)["block_shape"] and c["unfused"] and r(c)["route"] == 0]
    cond["the flag on a shape with no block form"] = [c for c in by["pfb_os"] if r(c)["flag_no_form"]]
    for c in cond["the flag on a shape with no block form"]:
        assert r(c)["route"] == (1 if r(c)["wave_shape"] and not c["unfused"] else 0), c
    assert any((c["M"], c["P"], 2 * c["H"]) == (1024, 16, 1024) and c["block"] and r(c)["route"] == 0 and c["units"] and not c["refusal"] for c in by["pfb_os"])
    assert {"hop", "taps", "m64"} <= {("m64" if c["M"] == 64 else "hop" if 2 * c["H"] != c["M"] else "taps" if c["P"] not in fz.BLOCK_TAPS else "other")
                                      for c in cond["the flag on a shape with no block form"]}
    seen2, other = {}, []
    for c in by["pfb_os"]:
        if r(c)["block_shape"]:
            k = plan_key(c)
            if seen2.get(k, set()) - {r(c)["route"]}:
                other.append(c)
            seen2.setdefault(k, set()).add(r(c)["route"])
    cond["a cached block plan met again on the other route"] = other
    cond["a reserve on route 2"] = [c for c in two if c["reserve"]]
    streams2 = [c for c in by["bank_streams"] if r(c)["route"] == 2]
    cond["bank_streams on route 2 with an odd number of rows in a piece"] = [c for c in streams2 if r(c)["odd_rows_piece"]]
    cond["bank_streams on a block plan sent down route 0"] = [c for c in by["bank_streams"] if r(c)["block_shape"] and c["unfused"]]
    counts = {k: len(v) for k, v in cond.items()}
    print(counts)
    short = {k: n for k, n in counts.items() if n < LEAST}
    assert not short, short
    for f in ONE_CALL:   # the staging size: a set test
        assert any(r(c)["staging"] == fz.STAGING and c["units"] and not c["refusal"] for c in by[f]), f
    # every case respects the bound that keeps the restatement fast
    for c in drawn:
        M, P, H = c["M"], c["P"], c["H"]
        window, hop, unit_out, min_rows = fz.cut_of(c["kind"], M, P, H)
        assert 1 <= H <= M and 1 <= P <= 20 and (M <= 300 or M in (512, 1024) or M == fz.STAGING), c
        assert (min_rows + 1) * M <= fs.POINTS, c
        if c["family"] == "bank_streams":
            assert c["n"] == sum(c["pieces"]) <= max(fs.transforms_allowed(M) * hop, 3 * window + hop), c
        else:
            G = fz.block_consts(M)[0] if r(c)["block_shape"] else 1   # the workgroup kernel: three workgroups of G streams of 64 rows
            assert c["units"] <= (3 if M == fz.STAGING else fs.transforms_allowed(M)) and c["units"] <= 3 * 64 * G + 20, c
            assert c["units"] == fz.units_of((window, hop), c["n"]) and r(c)["nout"] == c["units"] * unit_out, c
            T = c["units"] if c["family"] == "pfb_os" else c["units"] + min_rows - 1
            assert c["first_row"] + T <= fz.TOP, c   # never wraps past 2^64


def test_the_tools_cut_is_the_headers(drawn, emu):
    """what the tool computes for itself (cut_of, units_of, passes_of) against libredio_amd/csrc/pfb_bank_cut.h as tests/emu compiles it,
    on the drawn cases: the family's cut, the units of the call, the pass count and the short last pass; every pass's input and output
    offsets are its first unit times the hop and times the output per unit; a chunk below min_rows counts as min_rows"""
    import ctypes as C
    SZ = C.c_size_t
    emu.emu_bank_units.restype = SZ
    emu.emu_bank_units.argtypes = [C.POINTER(SZ), SZ]
    emu.emu_bank_cut.argtypes = [C.POINTER(SZ), SZ, SZ, C.POINTER(SZ)]
    emu.emu_bank_pass.argtypes = [C.POINTER(SZ), SZ, SZ, SZ, C.POINTER(SZ)]
    emu.emu_bank_cut_of.argtypes = [C.c_int, SZ, SZ, SZ, C.POINTER(SZ)]
    seen, below = set(), 0
    for c in drawn:
        kind, M, P, H, units = c["kind"], c["M"], c["P"], c["H"], c["units"]
        key = (kind, M, P, H, c["chunk"], units)
        if key in seen:
            continue
        seen.add(key)
        cut = fz.cut_of(kind, M, P, H)
        window, hop, unit_out, min_rows = cut
        c5, o3, o5 = (SZ * 5)(), (SZ * 3)(), (SZ * 5)()
        emu.emu_bank_cut_of(fz.STREAM_KINDS.index(kind), M, P, H, c5)
        assert list(c5) == [*cut, M], c
        assert emu.emu_bank_units(c5, c["n"]) == units == fz.units_of(cut, c["n"]), c
        if not units:
            continue
        emu.emu_bank_cut(c5, c["chunk"], units, o3)
        npass, last, per = fz.passes_of(cut, M, c["chunk"], units)
        assert o3[0] >= min_rows and o3[1] == per + min_rows - 1 and o3[2] == npass, (c, list(o3))
        below += 0 < c["chunk"] < min_rows and o3[0] == min_rows
        nxt = 0
        for i in sorted({0, 1, npass // 2, npass - 2, npass - 1} & set(range(npass))):
            emu.emu_bank_pass(c5, c["chunk"], units, i, o5)
            first, n, in_off, rows, out_off = o5
            assert first == i * per and n == (last if i == npass - 1 else per), (c, i, list(o5))
            assert (in_off, out_off, rows) == (first * hop, first * unit_out, n + min_rows - 1) and rows <= o3[1], (c, i, list(o5))
            assert in_off + (n - 1) * hop + window <= c["n"] and out_off + n * unit_out <= units * unit_out, (c, i, list(o5))
    assert len(seen) >= DRAWN // 2 and below >= LEAST, (len(seen), below)


def test_route_2_is_in_the_opening_rounds_of_the_gpu_runs():
    """tests/test_gpu_fuzz_banks.py runs the tool per family (--only) at SEED: the OPENING cases it runs whatever the machine's speed
    hold the workgroup kernel, on route 2 and sent down route 0, for the one-call family and for the streams"""
    for fam in ("pfb_os", "bank_streams"):
        gen = fz.Gen(SEED)
        opening = [gen.draw(f) for _, f in zip(range(fz.OPENING), fz.sequence(gen, fam))]
        assert any(c["route"]["route"] == 2 for c in opening), fam
        assert any(c["route"]["block_shape"] and c["unfused"] for c in opening), fam


def test_the_tools_block_geometry_is_the_headers(drawn):
    """block_consts and block_geometry against libredio_amd/csrc/pfb_os_p2_core.h as tests/emu_pfb_os_p2 compiles it, on the drawn
    route-2 cases: streams per workgroup, rows per iteration, and on devices of 1 to 304 CUs the rows per stream, the streams and
    the workgroups; the case's own record is the one for NOMINAL_CUS"""
    import ctypes as C
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "emu_pfb_os_p2"), "-s"])
    E = C.CDLL(os.path.join(ROOT, "tests", "_build", "libemu_pfb_os_p2.so"))
    for name, args in (("rows_per_stream", [C.c_long, C.c_long, C.c_int]), ("streams", [C.c_long, C.c_long]), ("groups", [C.c_long, C.c_long, C.c_int])):
        f = getattr(E, "emu_pfb_os_p2_" + name)
        f.argtypes, f.restype = args, C.c_long
    two = [c for c in drawn if c["route"]["route"] == 2]
    assert len(two) >= 5 * LEAST
    for c in two:
        M, rows = c["M"], c["units"]
        assert c["route"]["geometry"] == list(fz.block_geometry(M, rows, fz.NOMINAL_CUS)), c
        for cus in (1, 2, 8, 256, 304):
            G, TR, rps, streams, groups = fz.block_geometry(M, rows, cus)
            assert (G, TR) == (E.emu_pfb_os_p2_streams_per_group(M), E.emu_pfb_os_p2_rows_per_iter(M)) == p2.shape_consts(M), c
            assert rps == E.emu_pfb_os_p2_rows_per_stream(rows, cus, M) == p2.rows_per_stream(rows, cus, M) and rps % TR == 0, (c, cus)
            assert streams == E.emu_pfb_os_p2_streams(rows, rps) and groups == E.emu_pfb_os_p2_groups(rows, rps, M), (c, cus)
    # on one CU the drawn counts reach past one workgroup and leave a short last stream
    assert any(fz.block_geometry(c["M"], c["units"], 1)[4] > 1 for c in two) and any(c["units"] % 64 for c in two if c["units"] > 64)


# ---- the defining sums in float64, vectorised ----------------------------------------------------------------------------------------------
def exact_synth(X, h, M, P):
    """test_pfb_synth_cpu.py: y[t M + m] = sum_p v_{t+p}[m] h[M p + m], v_t the unnormalised inverse transform of row t"""
    T = len(X) // M
    V = np.fft.ifft(X[: T * M].astype(np.complex128).reshape(T, M), axis=1) * M
    g = h.astype(np.float64).reshape(P, M)
    return sum(V[p: T - P + 1 + p] * g[p] for p in range(P)).reshape(-1)


def exact_os(x, h, M, P, H, F, rows):
    """test_pfb_os_cpu.formula_f64, X_r[k] = sum_n h[n] x[r H + n] W^(k ((F + r) H + n)): the sum over n = M p + m folded over p first
    (W^(k M p) = 1), the factor W^(k s_r), s_r = ((F + r) H) mod M, taken out with its exponent reduced mod M exactly"""
    win = np.lib.stride_tricks.sliding_window_view(x.astype(np.complex128), M * P)[::H][:rows]
    u = (win * h.astype(np.float64)).reshape(rows, P, M).sum(axis=1)
    s = np.array([((F + r) % M) * H % M for r in range(rows)], np.int64)
    k = np.arange(M, dtype=np.int64)
    return (np.fft.fft(u, axis=1) * np.exp(-2j * np.pi * ((k[None, :] * s[:, None]) % M) / M)).reshape(-1)


def exact_os_synth(X, h, M, P, H, F):
    """test_pfb_os_synth_cpu.formula_f64, y[n] = sum_r w_r[tau mod M] h[tap(tau - (F + r) H)] over the rows whose offset lies in
    [0, P M): for output q H + j the rows r = q + k, k < L, at offset (L - 1 - k) H + j, one gather per k"""
    import pfb_os_synth_ref as ref
    T = len(X) // M
    L = ref.nrows_per_hop(M, P, H)
    hops = T - L + 1
    W = np.fft.ifft(X[: T * M].astype(np.complex128).reshape(T, M), axis=1) * M
    h = h.astype(np.float64)
    q, j = np.arange(hops, dtype=np.int64)[:, None], np.arange(H, dtype=np.int64)[None, :]
    col = ((((F + L - 1) % M) + q) * H + j) % M          # tau mod M
    y = np.zeros((hops, H), np.complex128)
    for k in range(L):
        o = (L - 1 - k) * H + j[0]
        ok = o < P * M
        taps = np.where(ok, h[np.where(ok, (P - 1 - o // M) * M + o % M, 0)], 0.0)
        y += W[q + k, col] * taps[None, :]
    return y.reshape(-1)


def exact(c, x, h):
    kind, M, P, H, F = c["kind"], c["M"], c["P"], c["H"], c["first_row"]
    if kind == "pfb_synth":
        return exact_synth(x, h, M, P)
    if kind == "pfb_os":
        return exact_os(x, h, M, P, H, F, c["units"])
    return exact_os_synth(x, h, M, P, H, F)


def test_the_vectorised_sums_are_the_loops_of_the_family_tests(oracle):
    """the two formula_f64 loops as their own test files write them, on small shapes: the vectorised forms above are the same sums"""
    from test_pfb_os_cpu import formula_f64 as os_loop
    from test_pfb_os_synth_cpu import formula_f64 as os_synth_loop
    for M, P, H, F in [(12, 3, 5, 3), (8, 2, 8, 1), (7, 3, 1, 0), (6, 1, 4, 2 ** 40 + 1)]:
        L = fz.nrows_per_hop(M, P, H)
        h = oracle.synth_f32(3, P, M * P)
        x = oracle.synth_iq(5, M, M * P + 8 * H)
        assert np.allclose(exact_os(x, h, M, P, H, F, 9), os_loop(x, h, M, H, F, 9).reshape(-1), rtol=0, atol=1e-10)
        X = oracle.synth_iq(6, M, (L + 8) * M)
        assert np.allclose(exact_os_synth(X, h, M, P, H, F), os_synth_loop(X, h, M, P, H, F), rtol=0, atol=1e-10)


def test_restatements_against_float64_on_the_generators_shapes(oracle):
    gen = fz.Gen(SEED)
    worst, checked, met = {}, 0, set()
    for _, fam in zip(range(DRAWN), fz.sequence(gen, None)):
        c = gen.draw(fam)
        nout = c["route"]["nout"]
        if not 1 <= nout <= MOST_VALUES or c.get("refusal"):
            continue
        if checked >= CHECKED and set(worst) >= set(fz.FAMILIES) and c["M"] not in {512, 1024} - met:
            continue   # behind the first CHECKED cases only what 512 and 1024 channels still lack
        h = fz.taps_of(oracle, c)
        x = fz.case_input(oracle, c, spiced=False)
        if fam == "bank_streams":   # the stream model's pieces, concatenated: the one call with first_row = 0
            model = fz.stream_model(c, h)
            cuts = np.concatenate([[0], np.cumsum(c["pieces"])]).astype(np.int64)
            got = np.concatenate([model.feed(x[lo:hi]) for lo, hi in zip(cuts[:-1], cuts[1:])])
        else:
            got = fz.reference(c, x, h)
        want = exact(c, x, h)
        assert got.shape == want.shape == (nout,), c
        err = float(np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30))
        tol = 2e-6 * max(1.0, fs.largest_prime_factor(c["M"]) / 8.0)
        w = worst.setdefault(fam, [0.0, 0.0, None])
        if err / tol > w[0]:
            w[:] = [err / tol, err, (c["M"], c["P"], c["H"])]
        assert err <= tol, (fam, err, tol, c)
        checked += 1
        met.add(c["M"])
        if c["M"] in (512, 1024):
            big = worst.setdefault(("channels", c["M"]), [0.0, 0.0, None])
            if err / tol > big[0]:
                big[:] = [err / tol, err, (fam, c["M"], c["P"], c["H"])]
        if checked >= CHECKED and set(worst) >= set(fz.FAMILIES) and {512, 1024} <= met:
            break
    big = {k: worst.pop(k) for k in list(worst) if isinstance(k, tuple)}
    for fam, (frac, err, shape) in sorted(worst.items()):
        print(f"{fam:12s} worst distance {err:.2e}, {frac:.2f} of its bound, at (M, P, H) = {shape}")
    for (_, M), (frac, err, shape) in sorted(big.items()):
        print(f"{M:4d} channels worst distance {err:.2e}, {frac:.2f} of its bound, at (family, M, P, H) = {shape}")
    assert checked >= 200 and set(worst) == set(fz.FAMILIES) and {512, 1024} <= met, (checked, sorted(worst), sorted(met))
