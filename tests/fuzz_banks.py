#!/usr/bin/env python3
"""Randomised differential run of the three two-pass filterbank plans against their bit-exact restatements (tests/pfb_synth_ref.py,
pfb_os_ref.py, pfb_os_synth_ref.py), beyond the fixed shapes of their own test files: the sibling of tests/fuzz_parity.py and
tests/fuzz_spectra.py for the synthesis bank redio_pfb_synth_*, the oversampled channelizer redio_pfb_os_* (its workgroup kernel, route 2,
included: REDIO_PFB_OS_BLOCK, one_kernel=True), the oversampled synthesis bank redio_pfb_os_synth_* and their three streams, all of
which run through one driver (libredio_amd/csrc/pfb_bank.hip).

    python tests/fuzz_banks.py [seconds] [seed] [--only FAMILY]     FAMILY: pfb_synth pfb_os pfb_os_synth bank_streams
    python tests/fuzz_banks.py --draw COUNT [seed] [--only FAMILY]  the cases a run would draw, one JSON line each; needs no GPU

A run first draws OPENING cases of every family, whatever the clock says, then draws families at random until the budget ends.  Plans are
cached by shape, and every case sets the driver's state (set_unfused, set_chunk_rows, reserve) itself, so a later call on a shape meets
the scratch an earlier call left under another route, chunk or length.  Prints one FAIL line per mismatch and a summary; exit status 1 on
any failure; the summary's `runs` counts the cases per family and, as "FAMILY route R", per family and route.  FUZZ_TRACE=file: what the
generator needs to draw the next case is written there before every case; FUZZ_STATE=file runs exactly that one case again.

A case is drawn completely (every seed included) before anything runs, and running it draws nothing more: the dry mode and a run see
the same sequence.  The route, the hop, the output length and the chunk cut of a case are computed here from the rules include/redio.h,
DESIGN.md and libredio_amd/csrc/pfb_bank_cut.h state, not asked of the library.

The helpers shared with the second tool (largest_prime_factor, transforms_allowed, spice, same_nan, check, SPECIALS, and the Runner's
dev / nans / plan) are fuzz_spectra's own: importing it imports neither torch nor the library."""
import json
import math
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import fuzz_spectra as fs  # noqa: E402

FAMILIES = ["pfb_synth", "pfb_os", "pfb_os_synth", "bank_streams"]
STREAM_KINDS = ["pfb_synth", "pfb_os", "pfb_os_synth"]     # SynthesizerStream, OversampledChannelizerStream, OversampledSynthesizerStream
OPENING = fs.OPENING   # cases per family before the clock is consulted
POOL = 12              # shapes kept per family for "the same shape again"
WAVE_M, WAVE_H, WAVE_TAPS = 64, 32, (4, 8, 16)   # the one-kernel shapes: 64 channels, 4 / 8 / 16 taps per branch, the oversampled plans at hop 32
# the oversampled channelizer's workgroup kernel (route 2, with the plan's one_kernel flag): these channel counts at hop M / 2 with
# the wave kernels' taps, 1024 x 16 left out (include/redio.h; tests/pfb_os_p2_ref.route)
BLOCK_M, BLOCK_TAPS, BLOCK_LEFT_OUT = (32, 128, 256, 512, 1024), WAVE_TAPS, ((1024, 16),)
BLOCK_MIN_ROWS = 64    # PFBOS_P2_MIN_ROWS: a row stream's floor
NOMINAL_CUS = 256      # the CU count the geometry of a route-2 case is recorded for (an MI355X's); the rule takes any
STAGING = 8194         # 2 17 241: a generic-radix stage beyond LDS, the transform needs a work buffer (tests/test_fft_route.py)
CHUNK_BYTES = 64 << 20  # route 0's default pass: 64 MiB of rows
CHUNK_KINDS = ["default", "min", "min+1", "min+small", "all", "below"]   # below: fewer rows than a pass needs count as min_rows
ERR_ARG = -1
TOP = (1 << 64) - 1


def nrows_per_hop(M, P, H):
    return -(-(M * P) // H)


def cut_of(fam, M, P, H):
    """(window, hop, unit_out, min_rows) in elements of the family's call, restated from pfb_bank_cut.h's table"""
    if fam == "pfb_synth":
        return M * P, M, M, P
    if fam == "pfb_os":
        return M * P, H, M, 1
    L = nrows_per_hop(M, P, H)
    return M * L, M, H, L


def units_of(cut, n_in):
    window, hop = cut[0], cut[1]
    return 0 if n_in < window else (n_in - window) // hop + 1


def passes_of(cut, M, asked, units):
    """(passes, units of the last pass, units per full pass) of a route-0 call: bank_chunk_rows, bank_pass_rows and bank_passes restated"""
    min_rows = cut[3]
    chunk = max(asked if asked else CHUNK_BYTES // (M * 8), min_rows)
    per = min(units + min_rows - 1, chunk) - min_rows + 1
    n = -(-units // per)
    return n, units - (n - 1) * per, per


def wave_shape(fam, M, P, H):
    return M == WAVE_M and P in WAVE_TAPS and (fam == "pfb_synth" or H == WAVE_H)


def block_shape(fam, M, P, H):
    """a shape with a workgroup form: what the plan's one_kernel flag turns into route 2"""
    return fam == "pfb_os" and M in BLOCK_M and P in BLOCK_TAPS and 2 * H == M and (M, P) not in BLOCK_LEFT_OUT


def block_consts(M):
    """(G, TR) of pfb_os_p2_core.h, restated: streams per workgroup, rows per stream and iteration"""
    return (1, 4096 // M) if M >= 256 else (256 // M, 16)


def block_geometry(M, rows, cus):
    """(G, TR, rows per stream, streams, workgroups) of a route-2 launch over `rows` rows on `cus` CUs, restated from
    pfb_os_p2_core.h: about four workgroups per CU, a multiple of the iteration's rows, at least the floor"""
    G, TR = block_consts(M)
    rps = -(-rows // (4 * cus * G))
    rps = max(-(-rps // TR) * TR, BLOCK_MIN_ROWS)
    streams = -(-rows // rps)
    return G, TR, rps, streams, -(-streams // G)


def is_prime(n):
    return n > 1 and fs.largest_prime_factor(n) == n


# ---- the generator --------------------------------------------------------------------------------------------------------------------------
class Gen:
    """rng: the seeded generator; pool: per family, the plan shapes drawn so far (a share of the cases draws one of them again)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.pool = {f: [] for f in FAMILIES}

    def state(self):
        return {"rng": self.rng.bit_generator.state, "pool": self.pool}

    def restore(self, st):
        self.rng.bit_generator.state = st["rng"]
        self.pool = {f: [dict(s) for s in st["pool"].get(f, [])] for f in FAMILIES}

    def i(self, lo, hi):
        return int(self.rng.integers(lo, hi))

    def p(self, prob):
        return bool(self.rng.random() < prob)

    def pick(self, seq):
        return seq[self.i(0, len(seq))]

    def seed(self):
        return self.i(1, 1 << 30)

    def shape_again(self, fam, fresh):
        """a plan shape of this family: one drawn before (a quarter of the time, once there is one) or a fresh one"""
        if self.pool[fam] and self.p(0.25):
            return dict(self.pick(self.pool[fam]))
        s = fresh()
        self.pool[fam].append(dict(s))
        del self.pool[fam][:-POOL]
        return s

    def hop(self, M, P, stream):
        """the oversampled plans' hop: 32 half the time at 64 channels, else the edges (M, M / 2, 1, M - 1), any value, one coprime to M,
        one in (M / 2, M); redrawn while L + 1 rows pass the restatement's size bound, so that H = 1 on a large M P stays cheap"""
        if M == STAGING:
            return self.pick([M, M // 2, self.i(M // 2 + 1, M)])
        while True:
            if M == WAVE_M and self.p(0.5):
                H = WAVE_H
            else:
                kind = self.i(0, 7)
                if kind == 5:      # coprime to M
                    H = next(h for h in range(self.i(1, M + 1), M + 2) if math.gcd(h, M) == 1)
                    H = H if H <= M else 1
                elif kind == 6:    # M / 2 < H < M, where there is such a value
                    H = self.i(M // 2 + 1, M) if M // 2 + 1 < M else M
                else:
                    H = [M, max(M // 2, 1), 1, max(M - 1, 1), self.i(1, M + 1)][kind]
            if (nrows_per_hop(M, P, H) + 1) * M * (3 if stream else 1) <= fs.POINTS:
                return H

    def block_flagged(self, fam):
        """a shape of the workgroup kernel with the flag set, 1024 x 16 (no workgroup form: route 0) among them.  The shares: a run
        of 6000 cases has some 1500 of pfb_os; 0.6 of its fresh shapes come from here, 24 in 25 of those have a workgroup form and
        0.7 of those calls stay on route 2 (driver_state), some 600 cases.  The rarest conditions on them are a refusal (0.15 of the
        calls with a row, some 80 cases), none or one row (0.07 each, 85), spiced (0.2 of the calls that are not refused, 95), the
        1024 channels (a fifth, less its 16 taps: 95) and a cached plan met again on the other route (a quarter of the cases draw an
        earlier shape, 0.42 of those pairs differ in route: 90), each above the 60 that are 1 % of a run.  Of the 500 bank_streams
        cases of this kind 0.6 come from here, 0.65 of those stay on route 2 (190) and 0.35 go down route 0 (100)."""
        M = self.pick(list(BLOCK_M))
        P = self.pick([4, 8, 4, 8, 16] if (M, 16) in BLOCK_LEFT_OUT else list(BLOCK_TAPS))   # 1024 x 16: a fifth of the 1024s
        taps = "lpf" if self.p(0.5) else "synth"
        return {"kind": fam, "M": M, "P": P, "H": M // 2, "fused": self.p(0.5), "taps": taps, "tseed": self.seed(), "block": True}

    def shape(self, fam, stream=False):
        if fam == "pfb_os" and self.p(0.6):
            return self.block_flagged(fam)
        r = self.rng.random()
        if r < 0.5:
            M = WAVE_M
        elif r < 0.53 and not stream:
            M = STAGING
        else:
            M = self.pick([32, 128, 256, 512, 1024, 100, 48, 12, 7, 2, 1, self.i(1, 301)])
        if M == STAGING:
            P = self.pick([1, 2, 3])
        elif M == WAVE_M and self.p(0.4):   # the wave kernels' taps more often than the list below gives them: with hop 32 half the time
            P = self.pick(list(WAVE_TAPS))  # and set_unfused on 0.4 of those, less leaves an oversampled family's wave route near 1 % of a run
        else:
            P = self.pick([4, 8, 16, 1, 2, 3, 5, self.i(1, 21)])
        H = M if fam == "pfb_synth" else self.hop(M, P, stream)
        taps = "lpf" if M * P >= 3 and self.p(0.5) else "synth"
        # the flag where there is no workgroup form (another hop, other taps, 64 channels) and, now and then, where there is one
        block = fam == "pfb_os" and self.p(0.3)
        return {"kind": fam, "M": M, "P": P, "H": H, "fused": self.p(0.5), "taps": taps, "tseed": self.seed(), "block": block}

    def driver_state(self, c, fam, units):
        """set_unfused, set_chunk_rows and reserve, drawn for every case: the plan is cached, so what an earlier case set is still there"""
        M, P, H = c["M"], c["P"], c["H"]
        min_rows = cut_of(fam, M, P, H)[3]
        wave = wave_shape(fam, M, P, H)
        blk = c["block"] and block_shape(fam, M, P, H)
        kind = self.pick(CHUNK_KINDS)
        chunk = {"default": 0, "min": min_rows, "min+1": min_rows + 1, "min+small": min_rows + self.i(2, 8),
                 "all": max(1, units + min_rows - 1 + self.i(0, 9)), "below": self.i(1, min_rows + 1)}[kind]
        stream = c.get("family") == "bank_streams"
        c.update(unfused=(wave and self.p(0.4)) or (blk and self.p(0.35 if stream else 0.3)), chunk_kind=kind, chunk=chunk, reserve=self.p(0.2))

    def one_call(self, fam):
        c = self.shape_again(fam, lambda: self.shape(fam))
        M, P, H = c["M"], c["P"], c["H"]
        window, hop, unit_out, min_rows = cut = cut_of(fam, M, P, H)
        wave = wave_shape(fam, M, P, H)
        blk = c["block"] and block_shape(fam, M, P, H)
        r = self.rng.random()
        if M == STAGING:
            units = self.i(0, 4)
        elif blk:   # the workgroup kernel's launch: G streams per workgroup, TR rows per iteration, a floor of 64 rows per stream
            G, TR = block_consts(M)
            if r < 0.14:       # no row and one row: 7 % each
                units = int(r >= 0.07)
            elif r < 0.5:      # either side of an iteration, of a stream's floor and of a workgroup of such streams
                units = self.pick([TR, BLOCK_MIN_ROWS, BLOCK_MIN_ROWS * G]) + self.i(-1, 2)
            else:              # up to past three workgroups, with a short last stream and a short last iteration
                units = self.i(0, 3 * BLOCK_MIN_ROWS * G + 21)
        elif r < 0.06:   # no unit and one unit: 6 % each, a uniform draw would leave them under 1 %
            units = 0
        elif r < 0.12:
            units = 1
        else:   # wave: several wavefronts of 64 units, a short last one, both tile parities
            units = self.i(0, 3 * 64 + 21) if wave else self.i(0, 41)
        units = min(units, fs.transforms_allowed(M))
        partial = self.i(0, hop) if self.p(0.5) else 0       # a trailing partial row / hop of input: ignored
        n = (units - 1) * hop + window + partial if units else self.i(0, window)
        T = units if fam == "pfb_os" else units + min_rows - 1   # rows the call touches: first_row + T never passes 2^64
        first = 0 if fam == "pfb_synth" else self.pick([0, 1, self.i(0, 1 << 32), (1 << 32) + 5, TOP - T])
        self.driver_state(c, fam, units)
        # an output range that overlaps the input range: REDIO_ERR_ARG, nothing written (more often on the workgroup kernel's shapes)
        refusal = units > 0 and self.p(0.15 if blk else 0.05)
        c.update(family=fam, units=units, n=n, first_row=first, in_base=8 * self.i(0, 2), out_base=8 * self.i(0, 2),
                 refusal=refusal, overlap=self.rng.random() if refusal else 0.0, out_first=refusal and self.p(0.5),
                 seed=self.seed(), spice=self.seed() if self.p(0.2 if blk else 0.12) else 0)
        c["route"] = route_of(c)
        return c

    def pfb_synth(self):
        return self.one_call("pfb_synth")

    def pfb_os(self):
        return self.one_call("pfb_os")

    def pfb_os_synth(self):
        return self.one_call("pfb_os_synth")

    def bank_streams(self):
        def fresh():
            return self.shape(self.pick(STREAM_KINDS), stream=True)
        c = self.shape_again("bank_streams", fresh)
        kind, M, P, H = c["kind"], c["M"], c["P"], c["H"]
        W, Hin = cut_of(kind, M, P, H)[:2]     # window and hop in input elements: (M P, M), (M P, H), (M L, M)
        most = max(fs.transforms_allowed(M) * Hin, 3 * W + Hin)
        # the pieces, by the rule of fuzz_spectra's pfb_streams: zero-length, shorter than a window, longer than two, anything
        pieces, pos = [], 0
        for _ in range(self.i(1, 9)):
            r = self.rng.random()
            if r < 0.15:
                ln = 0
            elif r < 0.45:
                ln = self.i(0, W)
            elif r < 0.65:
                ln = self.i(2 * W + 1, 3 * W + 2)
            else:
                ln = self.i(0, 2 * W + Hin)
            ln = min(ln, most - pos)
            pieces.append(ln)
            pos += ln
        again = sorted(self.i(0, pos + 1) for _ in range(self.i(0, 8))) if self.p(0.5) else None
        c["family"] = "bank_streams"
        self.driver_state(c, kind, units_of(cut_of(kind, M, P, H), pos))
        if c["chunk_kind"] == "all":   # a piece is no whole call: keep to the chunk settings that do not depend on the length
            c.update(chunk_kind="default", chunk=0)
        c.update(family="bank_streams", pieces=pieces, again=again, n=int(pos), units=units_of(cut_of(kind, M, P, H), pos), first_row=0,
                 seed=self.seed(), spice=self.seed() if self.p(0.12) else 0)
        c["route"] = route_of(c)
        made = [units_of(cut_of(kind, M, P, H), int(e)) for e in np.cumsum([0] + pieces)]
        c["route"].update(odd_rows_piece=any((b - a) % 2 for a, b in zip(made[:-1], made[1:])), zero_piece=0 in pieces, short_piece=any(0 < v < W for v in pieces), long_piece=any(v > 2 * W for v in pieces),
                          odd_piece=any(v % 2 for v in pieces), reset=again is not None)
        return c

    def draw(self, fam):
        return getattr(self, fam)()


def route_of(c):
    """what the driver does with this case, from the documented rules: the route (include/redio.h: 64 channels x 4 / 8 / 16 taps, the
    oversampled plans at hop 32; 2 the oversampled channelizer's workgroup shapes with the plan's flag; 0 after set_unfused), the
    launch geometry of route 2 on NOMINAL_CUS CUs, the output length, and on route 0 the cut of pfb_bank_cut.h"""
    fam, M, P, H, units = c["kind"], c["M"], c["P"], c["H"], c["units"]
    cut = cut_of(fam, M, P, H)
    wave = wave_shape(fam, M, P, H)
    blk = c["block"] and block_shape(fam, M, P, H)
    route = 0 if c["unfused"] else 1 if wave else 2 if blk else 0
    npass, last, per = passes_of(cut, M, c["chunk"], units) if units and route == 0 else (0, 0, 0)
    geometry = list(block_geometry(M, units, NOMINAL_CUS)) if route == 2 else None
    return {"wave_shape": wave, "block_shape": blk, "flag_no_form": c["block"] and not blk, "geometry": geometry, "route": route,
            "m64_generic": M == WAVE_M and not wave, "two_pass_shape": not wave and not blk, "nout": units * cut[2],
            "min_rows": cut[3], "passes": npass, "short_last": bool(npass >= 2 and last < per), "staging": M if M == STAGING else 0,
            "skips_oldest": bool(fam == "pfb_os_synth" and nrows_per_hop(M, P, H) * H > P * M)}


def sequence(gen, only):
    """the families for ever: the opening round of each, then families at random"""
    fams = [only] if only else FAMILIES
    for f in fams:
        for _ in range(OPENING):
            yield f
    while True:
        yield only if only else FAMILIES[gen.i(0, len(FAMILIES))]


def parse(argv):
    only, pos, draw = None, [], None
    it = iter(argv)
    for a in it:
        if a == "--only":
            only = next(it)
            assert only in FAMILIES, f"--only takes one of {FAMILIES}"
        elif a == "--draw":
            draw = int(next(it))
        else:
            pos.append(a)
    return only, draw, pos


# ---- a case's data and its reference: no torch, no library ------------------------------------------------------------------------------
def taps_of(O, c):
    return O.lpf_corrected(c["M"] * c["P"], 0.45 / c["M"]) if c["taps"] == "lpf" else O.synth_f32(c["tseed"], 0, c["M"] * c["P"])


def case_input(O, c, spiced=True):
    """the case's n cf32 input elements (a stream case: the whole stream), spiced where the case says so"""
    n = c["n"]
    return fs.spice(O.synth_iq(c["seed"], 0, max(n, 1))[:n], c["spice"] if spiced else 0)


def reference(c, x, h, first_row=None):
    """the restatement's flat output of one call on x"""
    import pfb_os_ref
    import pfb_os_synth_ref
    import pfb_synth_ref
    fam, M, P, H, ff = c["kind"], c["M"], c["P"], c["H"], c["fused"]
    F = c["first_row"] if first_row is None else first_row
    if fam == "pfb_synth":
        return pfb_synth_ref.synth(x, h, M, P, ff)
    if fam == "pfb_os":
        return pfb_os_ref.channelize(x, h, M, P, H, F, ff).reshape(-1)
    return pfb_os_synth_ref.synth(x, h, M, P, H, F, ff)


class SynthStreamModel:
    """redio_pfb_synth_stream_*: P - 1 whole rows and the values of a partial row carried (pfb_synth_ref.py has no model of its own; the
    two oversampled restatements do)"""

    def __init__(self, h, M, P, fused):
        self.h, self.M, self.P, self.fused = h, M, P, fused
        self.reset()

    def reset(self):
        self.tail = np.empty(0, np.complex64)

    @property
    def pending(self):
        return len(self.tail)

    def nout(self, n_new):
        import pfb_synth_ref
        return pfb_synth_ref.nout(len(self.tail) + n_new, self.M, self.P)

    def feed(self, X):
        import pfb_synth_ref
        buf = np.concatenate([self.tail, np.ascontiguousarray(X, np.complex64)])
        out = pfb_synth_ref.synth(buf, self.h, self.M, self.P, self.fused)
        self.tail = buf[(len(out) // self.M) * self.M:]
        return out


def stream_model(c, h):
    import pfb_os_ref
    import pfb_os_synth_ref
    kind, M, P, H, ff = c["kind"], c["M"], c["P"], c["H"], c["fused"]
    if kind == "pfb_synth":
        return SynthStreamModel(h, M, P, ff)
    return (pfb_os_ref if kind == "pfb_os" else pfb_os_synth_ref).StreamModel(h, M, P, H, ff)


# ---- running a case ------------------------------------------------------------------------------------------------------------------------
GUARD = 8   # cf32 elements of NaN in front of and behind every output


class Runner:
    dev, nans, plan = fs.Runner.dev, fs.Runner.nans, fs.Runner.plan   # the array at a byte offset of its allocation; NaN words; the plan cache

    def __init__(self):
        import torch
        import libredio_amd as R
        import oracle as O
        self.t, self.R, self.O = torch, R, O
        self.plans = {}

    def bank_plan(self, c, kind=None):
        R, kind = self.R, kind or c["kind"]
        cls = {"pfb_synth": R.Synthesizer, "pfb_os": R.OversampledChannelizer, "pfb_os_synth": R.OversampledSynthesizer, "pfb": R.Channelizer}[kind]
        hop = (c["H"],) if kind in ("pfb_os", "pfb_os_synth") else ()
        more = {"one_kernel": c["block"]} if kind == "pfb_os" else {}
        key = (cls.__name__, c["M"], c["P"], *hop, c["fused"], c["taps"], c["tseed"] if c["taps"] == "synth" else 0, *more.values())
        return self.plan(key, lambda: cls(taps_of(self.O, c), c["M"], c["P"], *hop, fused=c["fused"], **more))

    def set_state(self, plan, c):
        plan.set_unfused(c["unfused"])
        plan.set_chunk_rows(c["chunk"])
        self.reserved = None
        if c["reserve"]:
            count = self.R.lib().redio_malloc_count
            before = count()
            plan.reserve(c["n"])
            self.reserved = count()
            # routes 1 and 2 have no scratch: the reserve does nothing there (include/redio.h)
            assert not (c["kind"] == "pfb_os" and c["route"]["route"] and self.reserved != before), "a reserve on route 1 or 2 allocated"

    def after_reserve(self, c):
        """the oversampled channelizer's call behind a reserve of its length allocated nothing (route 0: the reserve took the scratch)"""
        return c["kind"] != "pfb_os" or self.reserved is None or self.R.lib().redio_malloc_count() == self.reserved

    def shape_answers(self, plan, c):
        """route, is_fused, hop and the output length against this tool's own arithmetic"""
        kind, r = c["kind"], c["route"]
        if plan.route != r["route"] or plan.is_fused != (r["route"] == 1):
            return ("route / is_fused", plan.route, plan.is_fused)
        if kind != "pfb_synth" and plan.hop != c["H"]:
            return ("hop", plan.hop)
        n = plan.nrows(c["n"]) * c["M"] if kind == "pfb_os" else plan.nout(c["n"])
        if n != r["nout"]:
            return ("nout / nrows", n, r["nout"])
        return None

    def guarded(self, nout, base):
        """a NaN-filled cf32 buffer and its view of nout elements `base` bytes past a 16-byte boundary, GUARD elements inside it"""
        t = self.t
        words = self.nans(2 * (nout + 2 * GUARD + 1))
        whole = t.view_as_complex(words.view(-1, 2))
        lo = GUARD + base // 8
        assert (whole.data_ptr() + 8 * lo) % 16 == base
        return whole, lo

    def call(self, plan, c, dx, out):
        return plan(dx, out=out) if c["kind"] == "pfb_synth" else plan(dx, first_row=c["first_row"], out=out)

    def refused(self, plan, c, x):
        """the input and the output in one buffer [pad | input | pad], the output laid over a part of what the call reads"""
        t, r = self.t, c["route"]
        cut = cut_of(c["kind"], c["M"], c["P"], c["H"])
        nout, read = r["nout"], (c["units"] - 1) * cut[1] + cut[0]
        pad = nout + 2
        buf = t.zeros(pad + len(x) + pad, dtype=t.complex64, device="cuda")
        dx = buf[pad: pad + len(x)]
        dx.copy_(t.from_numpy(x))
        if c["out_first"]:   # the output begins in front of the input and ends inside it
            start = pad - nout + 1 + int(c["overlap"] * min(nout, read))
        else:                # the output begins inside what the call reads
            start = pad + int(c["overlap"] * read)
        before = buf.clone()
        try:
            self.call(plan, c, dx, buf[start: start + nout])
            return False, "overlapping ranges were accepted"
        except self.R.RedioError as e:
            same = bool((t.view_as_real(buf).view(t.int32) == t.view_as_real(before).view(t.int32)).all().item())
            return e.code == ERR_ARG and same, ("refusal", e.code, same)

    def one_call(self, c):
        kind, M, P, r = c["kind"], c["M"], c["P"], c["route"]
        h = taps_of(self.O, c)
        x = case_input(self.O, c)
        plan = self.bank_plan(c)
        self.set_state(plan, c)
        bad = self.shape_answers(plan, c)
        if bad:
            return False, bad
        if c["refusal"]:
            return self.refused(plan, c, x)
        want = reference(c, x, h)
        if len(want) != r["nout"]:
            return False, ("the restatement's length", len(want), r["nout"])
        dx = self.dev(x, c["in_base"])
        assert not len(x) or dx.data_ptr() % 16 == c["in_base"]   # (an empty view reports no address of its own)
        whole, lo = self.guarded(len(want), c["out_base"])
        got = self.call(plan, c, dx, whole[lo: lo + len(want)]).reshape(-1)
        if not self.after_reserve(c):
            return False, "the call behind a reserve allocated"
        if got.numel() != len(want) or not fs.same_nan(got.cpu().numpy(), want):
            return False, "values"
        if not (fs.Runner.still_nan(self.t.view_as_real(whole[:lo])) and fs.Runner.still_nan(self.t.view_as_real(whole[lo + len(want):]))):
            return False, "wrote outside the output"
        if c["H"] == M and kind != "pfb_synth" and c["units"]:   # hop == nchan: the critically sampled plan's result, whatever first_row
            if kind == "pfb_os":
                twin = self.bank_plan(c, "pfb")(self.dev(x))
            else:
                base = self.bank_plan(c, "pfb_synth")   # shared with the pfb_synth cases: on its own route, at the default chunk
                base.set_unfused(False)
                base.set_chunk_rows(0)
                twin = base(self.dev(x))
            if not fs.same_nan(twin.reshape(-1)[: len(want)].cpu().numpy(), got.cpu().numpy()):
                return False, "hop == nchan against the " + ("Channelizer" if kind == "pfb_os" else "Synthesizer")
        return True, ""

    pfb_synth = pfb_os = pfb_os_synth = one_call

    def bank_streams(self, c):
        t, R, kind, M, n = self.t, self.R, c["kind"], c["M"], c["n"]
        h = taps_of(self.O, c)
        x = case_input(self.O, c)
        plan = self.bank_plan(c)
        self.set_state(plan, c)
        if plan.route != c["route"]["route"]:
            return False, ("route", plan.route)
        want = reference(c, x, h, first_row=0)
        model = stream_model(c, h)
        dx = self.dev(x)
        st = {"pfb_synth": R.SynthesizerStream, "pfb_os": R.OversampledChannelizerStream, "pfb_os_synth": R.OversampledSynthesizerStream}[kind](plan)
        cuts = np.concatenate([[0], np.cumsum(c["pieces"])]).astype(np.int64)
        for which, cuts in (("first pass", cuts), ("after reset", None if c["again"] is None else np.array([0] + c["again"] + [n], np.int64))):
            if cuts is None:
                break
            if which == "after reset":
                st.reset()
                model.reset()
                if st.pending != 0:
                    return False, "pending after reset"
            outs = []
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                lo, hi = int(lo), int(hi)
                expect = model.nout(hi - lo)
                if st.nout(hi - lo) != expect:
                    return False, (which, "nout", lo, hi)
                y = st(dx[lo:hi])
                piece = model.feed(x[lo:hi])
                if y.numel() != expect or len(piece) != expect:
                    return False, (which, "count", lo, hi)
                outs.append(y.clone())
                if st.pending != model.pending:
                    return False, (which, "pending", lo, hi, st.pending, model.pending)
            got = t.cat(outs).cpu().numpy() if outs else np.zeros(0, np.complex64)
            if not fs.same_nan(got, want):
                return False, which
        return True, ""

    def run(self, c):
        try:
            ok, why = getattr(self, c["family"])(c)
        except (AssertionError, self.R.RedioError) as e:   # a refused valid call or a host-side size check: a finding like any other
            ok, why = False, repr(e)
        self.t.cuda.synchronize()
        brief = {k: v for k, v in c.items() if k != "route"}
        fs.check(c["family"], ok, (why, json.dumps(brief)))
        per_route = f"{c['family']} route {c['route']['route']}"
        fs.runs[per_route] = fs.runs.get(per_route, 0) + 1


def main():
    only, draw, pos = parse(sys.argv[1:])
    if draw is not None:
        gen = Gen(int(pos[0]) if pos else 1)
        for _, fam in zip(range(draw), sequence(gen, only)):
            print(json.dumps(gen.draw(fam)))
        return 0
    budget = float(pos[0]) if pos else 60.0
    gen = Gen(int(pos[1]) if len(pos) > 1 else 1)
    trace, state = os.environ.get("FUZZ_TRACE"), os.environ.get("FUZZ_STATE")
    runner = Runner()
    if state:
        st = json.load(open(state))
        gen.restore(st)
        runner.run(gen.draw(st["family"]))
    else:
        t_end, ncases = None, 0
        opening = OPENING * (1 if only else len(FAMILIES))
        for fam in sequence(gen, only):
            if ncases == opening:
                t_end = time.time() + budget   # the opening round is outside the budget
            if t_end is not None and time.time() >= t_end:
                break
            ncases += 1
            if trace:
                with open(trace, "w") as fh:
                    json.dump(dict(gen.state(), family=fam), fh); fh.flush(); os.fsync(fh.fileno())
            runner.run(gen.draw(fam))
    print("runs", fs.runs, "failures", fs.fails)
    return 1 if fs.fails else 0


if __name__ == "__main__":
    sys.exit(main())
