#!/usr/bin/env python3
"""Randomised differential run of the real-input and spectrum plans against their bit-exact restatements (tests/fftr_ref.py,
ovsave_real_ref.py, pspec_ref.py, pspec_real_ref.py, pfb_pspec_ref.py), beyond the fixed shapes of their own test files: the sibling of
tests/fuzz_parity.py for redio_fftr_*, redio_ovsave_real_*, redio_pspec_* (cf32 and u8), redio_pspec_real_* and their streams, and for the
polyphase spectrometer redio_pfb_pspec_* (cf32 and u8; the 64-channel kernel, the workgroup kernel of REDIO_PFB_PSPEC_BLOCK and the
generic route) and its streams.

    python tests/fuzz_spectra.py [seconds] [seed] [--only FAMILY]     FAMILY: fftr ovsave_real pspec pspec_u8 pspec_real streams
                                                                              pfb_pspec pfb_streams
    python tests/fuzz_spectra.py --draw COUNT [seed] [--only FAMILY]  the cases a run would draw, one JSON line each; needs no GPU

A run first draws OPENING cases of every family, whatever the clock says, then draws families at random until the budget ends.  Plans are
cached by shape, so a later call on a shape meets the scratch an earlier call left.  Prints one FAIL line per mismatch and a summary;
exit status 1 on any failure; the summary's `runs` counts the cases per family and, for the polyphase spectrometer, as "FAMILY route R"
per family and route.  FUZZ_TRACE=file: what the generator needs to draw the next case is written there before every case;
FUZZ_STATE=file runs exactly that one case again.

A case is drawn completely (every seed included) before anything runs, and running it draws nothing more: the dry mode and a run see
the same sequence.  The route predicates of a case are computed here from the rules include/redio.h and DESIGN.md state, not asked of
the library."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

FAMILIES = ["fftr", "ovsave_real", "pspec", "pspec_u8", "pspec_real", "streams", "pfb_pspec", "pfb_streams"]
OPENING = 24           # cases per family before the clock is consulted
POINTS = 1 << 18       # transforms per case times N, at most (the large staging sizes excepted: one or two transforms)
WORK = 1 << 25         # the same times the largest prime factor: the restatement's generic-radix stage costs that much
SEG = 16               # REDIO_PSPEC_SEG
SPLIT_ROWS = 2048      # PSPEC_SPLIT_ROWS, PSPEC_REAL_SPLIT_ROWS: auto takes a wave per segment below this many rows
ERR_ARG = -1
ROUGH_EVEN = [14, 22, 34, 94, 442, 614, 2002, 1994, 3758, 5042, 7978]          # 2 x prime and the like
ODD_SIZES = [1, 3, 5, 7, 11, 13, 17, 97, 127, 251, 509, 1021, 1000, 96, 625, 3125, 2187, 1215]
STAGING = {"pspec": (65536, 8194), "pspec_u8": (65536, 8194), "pspec_real": (131072,), "fftr": (16388, 65536)}
PFB_M = 64                                # the polyphase spectrometer's one-kernel channel count, with PFB_TAPS taps per branch
PFB_TAPS = (4, 8, 16)
PFB_ONE_KERNEL = (32, 128, 256, 512, 1024)   # channel counts the inner channelizer runs as one kernel (with PFB_TAPS), not as two passes
PFB_BLOCK_MIN_ROWS = 64                   # PFBSPEC_P2_MIN_ROWS: a row stream of the workgroup kernel (route 2) sums at least this many rows
PFB_BLOCK_SPLIT_GROUPS_PER_CU = 2         # PFBSPEC_P2_SPLIT_GROUPS_PER_CU: route 2's auto mode is rows mode from this many workgroups per CU
NOMINAL_CUS = 256                         # the CU count a route-2 case's geometry is recorded for (an MI355X's); the rule takes any
PFB_SPLIT_WAVES = 1024                    # PFBSPEC_SPLIT_WAVES: auto lets a wave own whole rows from this many waves of ceil(64 / K) rows


def largest_prime_factor(n):
    p, m, f = 1, n, 2
    while f * f <= m:
        while m % f == 0:
            p, m = f, m // f
        f += 1
    return max(p, m) if m > 1 else p


def transforms_allowed(ncplx):
    """how many transforms of `ncplx` complex points a case may ask of the restatement"""
    return max(1, min(POINTS // max(ncplx, 1), WORK // (max(ncplx, 1) * largest_prime_factor(max(ncplx, 1)))))


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

    # small helpers over the generator
    def i(self, lo, hi):
        return int(self.rng.integers(lo, hi))

    def p(self, prob):
        return bool(self.rng.random() < prob)

    def pick(self, seq):
        return seq[self.i(0, len(seq))]

    def seed(self):
        return self.i(1, 1 << 30)

    def smooth_even(self, lim):
        while True:
            n = 2 ** self.i(1, 14) * 3 ** self.i(0, 6) * 5 ** self.i(0, 4)
            if n <= lim:
                return n

    def even_size(self, lim=8192):
        r = self.rng.random()
        if r < 0.45:
            return self.smooth_even(lim)
        if r < 0.65:
            return self.pick(ROUGH_EVEN)
        if r < 0.8:
            return self.pick([2, 4, 6, 8, 16, 64, 128, 512, 1024, 4096, 8192, 2000, 1000])
        return 2 * self.i(1, lim // 2 + 1)

    def shape_again(self, fam, fresh):
        """a plan shape of this family: one drawn before (a quarter of the time, once there is one) or a fresh one"""
        if self.pool[fam] and self.p(0.25):
            return dict(self.pick(self.pool[fam]))
        s = fresh()
        self.pool[fam].append(dict(s))
        del self.pool[fam][:-12]
        return s

    def spiced(self, prob=0.12):
        return self.seed() if self.p(prob) else 0

    # -- the families --
    def fftr(self):
        def fresh():
            r = self.rng.random()
            N = 2048 if r < 0.33 else 16388 if r < 0.36 else 65536 if r < 0.39 else self.even_size()
            return {"N": N, "inverse": self.p(0.5)}
        c = self.shape_again("fftr", fresh)
        N, inv = c["N"], c["inverse"]
        big = N in STAGING["fftr"]
        nb = self.i(1, 3) if big else min(self.i(1, 21), transforms_allowed(N // 2))
        nbins = N // 2 + 1
        strided = self.p(0.5)
        in_stride, out_stride = (nbins, N) if inv else (N, nbins)
        refusal = False
        if strided:
            gap_real, gap_spec = 2 * self.i(0, 9), self.i(0, 6)
            if inv:
                in_stride, out_stride = nbins + gap_spec, N + gap_real
            else:
                overlap = N > 2 and self.p(0.5)
                in_stride, out_stride = (2 * self.i(1, N // 2) if overlap else N + gap_real), nbins + gap_spec
            if self.p(0.2):   # an odd real-side stride: REDIO_ERR_ARG, nothing written
                refusal = True
                if inv:
                    out_stride += 1
                else:
                    in_stride += 1
        c.update(family="fftr", rows=nb, strided=strided, in_stride=in_stride, out_stride=out_stride, refusal=refusal,
                 seed=self.seed(), spice=self.spiced())
        c["route"] = {"fused": N == 2048, "strided": strided, "overlap": strided and not inv and in_stride < N, "refusal": refusal,
                      "staging": N if big else 0}
        return c

    def ovsave_real(self, fam="ovsave_real"):
        def fresh():
            N = 2048 if self.p(0.33) else self.even_size()
            k = self.pick([1, 2, 3, N - 1, self.i(1, N), self.i(1, N), 2 * self.i(1, N // 2 + 1)])
            k = max(1, min(k, N - 1))
            return {"N": N, "ntaps": k, "taps": "lpf" if k >= 3 and self.p(0.5) else "synth", "tseed": self.seed()}
        c = self.shape_again(fam, fresh)
        N, k = c["N"], c["ntaps"]
        hop = N - (k | 1) + 1
        blocks = min(self.i(0, 13), transforms_allowed(N // 2) // 2)
        n = N + (blocks - 1) * hop + self.i(0, hop) if blocks else self.i(0, N)
        c.update(family="ovsave_real", rows=blocks, n=n, seed=self.seed(), spice=self.spiced())
        c["route"] = {"fused": N == 2048, "ntaps_even": k % 2 == 0}
        return c

    def _pspec_shape(self, fam, real, stream=False):
        r = self.rng.random()
        fused_n = 2048 if real else 1024
        big = STAGING[fam]
        if r < 0.4:
            N = fused_n
        elif r < 0.4 + 0.02 * len(big) and not stream:
            N = self.pick(list(big))
        elif real:
            N = self.even_size()
        else:
            N = self.pick([self.i(1, 8193), self.i(1, 300), self.pick(ODD_SIZES), self.even_size(), 2048, 4096, 2048, 4096])
        K = self.pick([1, 2, 15, 16, 17, 31, 32, 33, 40, self.i(1, 71)])
        kind = self.i(0, 7)
        if N in big:
            K, kind = self.i(1, 3), self.pick([0, 0, 1])
        step = [N, N, max(1, N // 2), 1, self.i(1, max(N, 2)), self.i(N + 1, 3 * N + 1), self.i(N + 1, 3 * N + 1)][kind]
        if stream and self.p(0.2):
            step = self.i(N + 1, 3 * N + 1)
        window = self.pick(["none", "none", "lpf", "synth"])
        if window == "lpf" and N < 3:
            window = "synth"
        ncplx = N // 2 if real else N
        K = min(K, transforms_allowed(ncplx))
        if stream:   # a stream case needs a piece longer than two windows: (3 W + H) / step transforms within the bound
            while ((3 * ((K - 1) * step + N) + K * step) // step + 1) > transforms_allowed(ncplx):
                if K > 1:
                    K //= 2
                elif step < N:
                    step = min(N, 2 * step)
                else:
                    break
        return {"N": N, "K": K, "step": step, "window": window, "wseed": self.seed()}

    def _pspec_case(self, fam, real):
        c = self.shape_again(fam, lambda: self._pspec_shape(fam, real))
        N, K, step = c["N"], c["K"], c["step"]
        W, H = (K - 1) * step + N, K * step
        cap = transforms_allowed(N // 2 if real else N) // K
        rows = 1 if N in STAGING[fam] else min(self.i(0, 6), cap)
        n = W + (rows - 1) * H + self.i(0, min(H, 3000)) if rows else self.i(0, W)
        c.update(family=fam, rows=rows, n=n, mode=self.i(0, 3), seed=self.seed(), spice=0 if fam == "pspec_u8" else self.spiced())
        c["route"] = pspec_route(fam, c)
        return c

    def pspec(self):
        return self._pspec_case("pspec", False)

    def pspec_u8(self):
        c = self._pspec_case("pspec_u8", False)
        c.update(base=2 * self.i(0, 8), u8_first=self.p(0.5))
        c["route"]["base"] = c["base"]
        return c

    def pspec_real(self):
        c = self._pspec_case("pspec_real", True)
        c["base"] = 4 * self.i(0, 2)
        c["route"]["base"] = c["base"]
        return c

    def streams(self):
        kind = self.pick(["pspec", "pspec_u8", "pspec_real", "ovsave_real"])
        if kind == "ovsave_real":
            c = self.ovsave_real("streams")
            c = {k: c[k] for k in ("N", "ntaps", "taps", "tseed")}
            W, H = c["N"], c["N"] - (c["ntaps"] | 1) + 1
            most = max(transforms_allowed(c["N"] // 2) // 2, 4) * H + W
            route = {"fused": c["N"] == 2048, "ntaps_even": c["ntaps"] % 2 == 0, "H>W": False}
        else:
            real = kind == "pspec_real"
            c = self._pspec_shape(kind, real, stream=True)
            W, H = (c["K"] - 1) * c["step"] + c["N"], c["K"] * c["step"]
            most = max(transforms_allowed(c["N"] // 2 if real else c["N"]) * c["step"], 3 * W + H)
            route = pspec_route(kind, dict(c, rows=1, mode=0))
        # the pieces: zero-length, shorter than a window, longer than two, anything; with H > W also one that ends inside the skipped gap
        pieces, pos = [], 0
        for _ in range(self.i(1, 9)):
            r = self.rng.random()
            if r < 0.15:
                ln = 0
            elif r < 0.45:
                ln = self.i(0, W)
            elif r < 0.65:
                ln = self.i(2 * W + 1, 3 * W + 2)
            elif r < 0.8 and H > W:
                u = pos // H + self.i(0, 2)
                ln = max(0, u * H + W + self.i(0, H - W) - pos)
            else:
                ln = self.i(0, 2 * W + H)
            ln = min(ln, most - pos)
            pieces.append(ln)
            pos += ln
        again = sorted(self.i(0, pos + 1) for _ in range(self.i(0, 8))) if self.p(0.5) else None
        ends = np.cumsum(pieces)
        route.update(zero_piece=0 in pieces, short_piece=any(0 < v < W for v in pieces), long_piece=any(v > 2 * W for v in pieces),
                     odd_piece=any(v % 2 for v in pieces), ends_in_gap=bool(H > W and any(e % H >= W for e in ends[:-1])), reset=again is not None)
        c.update(family="streams", kind=kind, pieces=pieces, again=again, rows=int(pos), seed=self.seed(),
                 spice=0 if kind == "pspec_u8" else self.spiced(), route=route)
        return c

    # -- the polyphase spectrometer --
    def _pfb_shape(self, stream=False):
        # half of the shapes have 64 channels and four calls in five name their split mode: with K > 16 on about 0.58 of the shapes and the
        # fused taps on 0.79, less would leave "fused, K > 16, mode 1" (and mode 2) under 1 % of a run's cases.  Auto, at the row
        # counts of this tool, is the route of mode 2 (its threshold is test_gpu_pfb_pspec_launch.py's).
        # The workgroup kernel (route 2: the plan's flag on a one-kernel shape of the inner channelizer): a family has some 750 of a run's
        # 6000 cases, so a condition that must hold in 60 of them needs 8 % of its family.  Of the 0.45 without 64 channels 0.85 have a
        # workgroup channel count, 0.9 of those the kernel's taps and 0.8 of those the flag: some 205 route-2 cases per family -- 68 per
        # split mode (drawn evenly there), 40 per channel count and family, 72 spiced (0.35 there), and 50 per family on the same shapes
        # without the flag, down the generic route.  The two-pass shapes keep some 80 per family.
        if self.p(0.55):
            M = PFB_M
        elif self.p(0.85):
            M = self.pick(list(PFB_ONE_KERNEL))
        else:
            M = self.pick([100, 7, 48, self.i(1, 300)])
        if M in PFB_ONE_KERNEL and self.p(0.6):
            P = self.pick(list(PFB_TAPS))
        else:
            P = self.pick([4, 8, 16, self.i(1, 20)])
        block = self.p(0.8 if M in PFB_ONE_KERNEL and P in PFB_TAPS else 0.2)   # elsewhere the flag changes nothing
        K = min(self.pick([1, 2, 15, 16, 17, 31, 32, 33, 40, self.i(1, 71)]), transforms_allowed(M))
        while stream and K > 1 and 3 * (K - 1 + P) + K + 1 > transforms_allowed(M):   # a piece longer than two windows stays within the bound
            K //= 2
        taps = "lpf" if M * P >= 3 and self.p(0.5) else "synth"
        return {"M": M, "P": P, "K": K, "fir_fused": self.p(0.5), "taps": taps, "tseed": self.seed(), "block": block}

    def pfb_pspec(self):
        c = self.shape_again("pfb_pspec", self._pfb_shape)
        M, P, K = c["M"], c["P"], c["K"]
        W, H = (K - 1 + P) * M, K * M
        fused = M == PFB_M and P in PFB_TAPS
        two = pfb_route_number(c) == 2
        if two:   # the workgroup kernel: up to past three workgroups of G streams of ceil(64 / K) rows, and a short last stream
            rows = self.i(0, 3 * pfb_block_consts(M)[0] * -(-PFB_BLOCK_MIN_ROWS // K) + 3)
        else:
            rows = self.i(0, 3 * -(-64 // K) + 3) if fused else self.i(0, 6)   # fused: several wavefronts of ceil(64 / K) rows and a short last one
        rows = min(rows, transforms_allowed(M) // K)
        n = W + (rows - 1) * H + self.i(0, H) if rows else self.i(0, W)
        c.update(family="pfb_pspec", rows=rows, n=n, mode=self.pick([0, 1, 2] if two else [0, 1, 1, 2, 2]), base=2 * self.i(0, 8), cbase=8 * self.i(0, 2),
                 u8_first=self.p(0.5), seed=self.seed(), spice=self.spiced(0.35 if two else 0.12))
        c["route"] = pfb_route(c)
        return c

    def pfb_streams(self):
        c = self.shape_again("pfb_streams", lambda: self._pfb_shape(stream=True))
        M, P, K = c["M"], c["P"], c["K"]
        W, H = (K - 1 + P) * M, K * M
        most = max(transforms_allowed(M) * M, 3 * W + H)
        u8 = self.p(0.5)
        # the pieces, by the rule of `streams`: zero-length, shorter than a window, longer than two, anything (H <= W: no skipped gap)
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
                ln = self.i(0, 2 * W + H)
            ln = min(ln, most - pos)
            pieces.append(ln)
            pos += ln
        again = sorted(self.i(0, pos + 1) for _ in range(self.i(0, 8))) if self.p(0.5) else None
        route = {k: v for k, v in pfb_route(dict(c, rows=1, mode=0, base=0, cbase=0)).items() if k not in ("mode", "split", "base", "cbase", "geometry")}
        route.update(u8=u8, zero_piece=0 in pieces, short_piece=any(0 < v < W for v in pieces), long_piece=any(v > 2 * W for v in pieces),
                     odd_piece=any(v % 2 for v in pieces), reset=again is not None)
        c.update(family="pfb_streams", u8=u8, pieces=pieces, again=again, rows=int(pos), seed=self.seed(),
                 spice=0 if u8 else self.spiced(0.35 if route["route"] == 2 else 0.12),
                 route=route)
        return c

    def draw(self, fam):
        return getattr(self, fam)()


def pspec_route(fam, c):
    """the driver's route for this call, from the documented rules (include/redio.h)"""
    real = fam == "pspec_real"
    N, K, step = c["N"], c["K"], c["step"]
    S = (K + SEG - 1) // SEG
    fused = N == (2048 if real else 1024)
    split = S >= 2 and (not fused or c["mode"] == 2 or (c["mode"] == 0 and c["rows"] < SPLIT_ROWS))
    return {"fused": fused, "packs": c["window"] != "none" or step != N, "segments2": S >= 2, "mode": c["mode"], "split": bool(split),
            "H>W": step > N, "odd_step": step % 2 == 1, "fft_u8": N if fam == "pspec_u8" and N in (2048, 4096) else 0,
            "staging": N if N in STAGING.get(fam, ()) else 0}


def pfb_route_number(c):
    """redio_pfb_pspec_route by the rule of include/redio.h: 1 the 64-channel wave kernel, 2 the workgroup kernel (the plan's flag on 32,
    128, 256, 512 or 1024 channels with the same taps), 0 generic"""
    if c["M"] == PFB_M and c["P"] in PFB_TAPS:
        return 1
    return 2 if c["block"] and c["M"] in PFB_ONE_KERNEL and c["P"] in PFB_TAPS else 0


def pfb_block_consts(M):
    """(G, TR) of pfb_pspec_p2_core.h, restated: streams per workgroup, channelizer rows per stream and iteration"""
    return (1, 4096 // M) if M >= 256 else (256 // M, 16)


def pfb_block_geometry(M, K, rows, mode, cus):
    """a route-2 launch over `rows` output rows on `cus` CUs, restated from pfb_pspec_p2_core.h: whether a stream owns runs of segments
    (split), the units (rows, or segments), the units per stream (aiming at 4 cus G streams, at least 64 channelizer rows of full
    units), the streams and the workgroups"""
    G, TR = pfb_block_consts(M)
    least_rows = -(-PFB_BLOCK_MIN_ROWS // K)
    split = K > SEG and (mode == 2 or (mode == 0 and rows < PFB_BLOCK_SPLIT_GROUPS_PER_CU * cus * G * max(-(-1 // (4 * cus * G)), least_rows)))
    units = rows * (-(-K // SEG)) if split else rows
    ups = max(-(-units // (4 * cus * G)), -(-PFB_BLOCK_MIN_ROWS // (SEG if split else K)))
    streams = -(-units // ups)
    return {"G": G, "TR": TR, "split": bool(split), "units": units, "ups": ups, "streams": streams, "groups": -(-streams // G)}


def pfb_route(c):
    """the polyphase spectrometer's route for this call, from the documented rules (include/redio.h)"""
    M, P, K = c["M"], c["P"], c["K"]
    fused = M == PFB_M and P in PFB_TAPS
    one_kernel = M in PFB_ONE_KERNEL and P in PFB_TAPS
    number = pfb_route_number(c)
    geometry = pfb_block_geometry(M, K, c["rows"], c["mode"], NOMINAL_CUS) if number == 2 else None
    split = K > SEG and (not fused or c["mode"] == 2 or (c["mode"] == 0 and c["rows"] < PFB_SPLIT_WAVES * -(-64 // K)))
    if number == 2:
        split = geometry["split"]
    return {"route": number, "flag_no_form": c["block"] and number != 2, "geometry": geometry,
            "fused": fused, "one_kernel": one_kernel, "two_pass": not fused and not one_kernel, "m64_generic": M == PFB_M and not fused,
            "segments2": K > SEG, "mode": c["mode"], "split": bool(split), "fir_fused": c["fir_fused"], "base": c["base"], "cbase": c["cbase"]}


def sequence(gen, only):
    """(family, first of its opening round?) for ever: the opening round, then families at random"""
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


# ---- running a case ------------------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, 1e-30, -1e-30, 1e30, -1e30, 3e38, -3e38, np.inf, -np.inf, np.nan, 1.0, -1.0, 2.0 ** -126, 2.0 ** 127], np.float32)
fails, runs = 0, {}


def spice(x, seed):
    """seed != 0: signed zeros, subnormals, huge and tiny magnitudes (and, half of those times, inf / NaN) over a random share of the words"""
    if not seed or x.size == 0:
        return x
    r = np.random.default_rng(seed)
    w = x.view(np.float32).reshape(-1)
    pool = SPECIALS if r.random() < 0.5 else SPECIALS[np.isfinite(SPECIALS)]
    k = max(1, int(len(w) * 10.0 ** -r.uniform(0.3, 4.0)))
    w[r.integers(0, len(w), k)] = pool[r.integers(0, len(pool), k)]
    runs["spiced"] = runs.get("spiced", 0) + 1
    return x


def same_nan(got, want):
    """identical bits wherever the restatement's value is not a NaN, a NaN exactly where it has one (payloads differ between x86 and gfx950)"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape:
        return False
    g, w = got.view(np.float32).reshape(-1), want.view(np.float32).reshape(-1)
    wn = np.isnan(w)
    if not wn.any():
        return np.array_equal(g.view(np.uint32), w.view(np.uint32))
    return np.array_equal(np.isnan(g), wn) and np.array_equal(g.view(np.uint32)[~wn], w.view(np.uint32)[~wn])


def check(name, ok, detail):
    global fails
    runs[name] = runs.get(name, 0) + 1
    if not ok:
        fails += 1
        print("FAIL", name, detail, flush=True)


def window_of(O, c):
    if c["window"] == "none":
        return None
    return O.lpf_corrected(c["N"], 0.1) if c["window"] == "lpf" else O.synth_f32(c["wseed"], 0, c["N"])


def taps_of(O, c):
    return O.lpf_corrected(c["ntaps"], 0.08) if c["taps"] == "lpf" else O.synth_f32(c["tseed"], 0, c["ntaps"])


def case_input(O, c, spiced=True):
    """the case's input as the device gets it: f32 or cf32 samples, or the raw bytes of the u8 kinds"""
    fam = c["kind"] if c["family"] == "streams" else c["family"]
    sp = c["spice"] if spiced else 0
    if fam == "fftr":
        nin = c["N"] // 2 + 1 if c["inverse"] else c["N"]
        span = (c["rows"] - 1) * c["in_stride"] + nin + (1 if c["refusal"] else 0)
        return spice((O.synth_iq if c["inverse"] else O.synth_f32)(c["seed"], 0, span), sp)
    n = c["rows"] if c["family"] == "streams" else c["n"]
    if fam == "pspec_u8":
        return np.random.default_rng(c["seed"]).integers(0, 256, 2 * n, dtype=np.uint8)
    return spice((O.synth_iq if fam == "pspec" else O.synth_f32)(c["seed"], 0, max(n, 1))[:n], sp)


def pfb_taps_of(O, c):
    return O.lpf_corrected(c["M"] * c["P"], 0.45 / c["M"]) if c["taps"] == "lpf" else O.synth_f32(c["tseed"], 0, c["M"] * c["P"])


def pfb_input(O, c, u8, spiced=True):
    """a polyphase case's input: cf32 samples (spiced where the case says so) or the raw I/Q bytes; a stream case has `rows` samples"""
    n = c["rows"] if c["family"] == "pfb_streams" else c["n"]
    if u8:
        return np.random.default_rng(c["seed"]).integers(0, 256, 2 * n, dtype=np.uint8)
    return spice(O.synth_iq(c["seed"], 0, max(n, 1))[:n], c["spice"] if spiced else 0)


def samples_of(O, raw):
    return O.data_to_samples(raw) if len(raw) else np.zeros(0, np.complex64)


class Runner:
    def __init__(self):
        import torch
        import libredio_amd as R
        import oracle as O
        import fftr_ref, ovsave_real_ref, pspec_ref, pspec_real_ref, pfb_pspec_ref
        self.t, self.R, self.O = torch, R, O
        self.fftr_ref, self.ovsave_real_ref, self.pspec_ref, self.pspec_real_ref = fftr_ref, ovsave_real_ref, pspec_ref, pspec_real_ref
        self.pfb_pspec_ref = pfb_pspec_ref
        self.plans = {}

    def plan(self, key, make):
        """plans cached by shape (the newest 48): a later call meets the scratch an earlier one left"""
        if key not in self.plans:
            if len(self.plans) >= 48:
                self.plans.pop(next(iter(self.plans)))
            self.plans[key] = make()
        return self.plans[key]

    def pspec_plan(self, c, real):
        cls = self.R.PowerSpectrumReal if real else self.R.PowerSpectrum
        key = (cls.__name__, c["N"], c["K"], c["step"], c["window"], c["wseed"] if c["window"] == "synth" else 0)
        return self.plan(key, lambda: cls(c["N"], c["K"], c["step"], window_of(self.O, c)))

    def ovsave_plan(self, c):
        return self.plan(("OverlapSaveReal", c["N"], c["ntaps"], c["taps"], c["tseed"]), lambda: self.R.OverlapSaveReal(taps_of(self.O, c), c["N"]))

    def dev(self, a, base=0):
        """the array on the device, starting `base` bytes into its (256-byte aligned) allocation; never a null pointer"""
        t = self.t
        a = np.ascontiguousarray(a)
        raw = t.empty(a.nbytes + 16 + base, dtype=t.uint8, device="cuda")
        assert raw.data_ptr() % 16 == 0
        view = raw[base: base + a.nbytes]
        if a.nbytes:
            view.copy_(t.from_numpy(a.view(np.uint8).reshape(-1)))
        return view.view({np.dtype(np.float32): t.float32, np.dtype(np.complex64): t.complex64, np.dtype(np.uint8): t.uint8}[a.dtype])

    def nans(self, n):
        return self.t.full((n,), float("nan"), dtype=self.t.float32, device="cuda")

    @staticmethod
    def still_nan(t):
        return bool(t.isnan().all().item()) if t.numel() else True

    # -- the families --
    def fftr(self, c):
        t, ref = self.t, self.fftr_ref
        N, inv, nb, ins, outs = c["N"], c["inverse"], c["rows"], c["in_stride"], c["out_stride"]
        nbins = N // 2 + 1
        nin, nout = (nbins, N) if inv else (N, nbins)
        x = case_input(self.O, c)
        plan = self.plan(("Fftr", N, inv), lambda: self.R.Fftr(N, inv))
        dx = self.dev(x)
        count = (nb - 1) * outs + nout + 8
        words = self.nans(count if inv else 2 * count)          # NaN in every f32 word: the rows' gaps and a guard behind the last row
        out = words if inv else t.view_as_complex(words.view(-1, 2))
        if c["refusal"]:
            try:
                plan.strided(dx, nb, ins, outs, out=out)
                return False, "an odd real-side stride was accepted"
            except self.R.RedioError as e:
                return e.code == ERR_ARG and self.still_nan(words), ("refusal", e.code)
        if c["strided"]:
            plan.strided(dx, nb, ins, outs, out=out)
        else:
            plan(dx, out=out)
        got = out.cpu().numpy()
        one = ref.fftri if inv else ref.fftr
        ok, seen = True, np.zeros(len(got), bool)
        for b in range(nb):
            ok = ok and same_nan(got[b * outs: b * outs + nout], one(x[b * ins: b * ins + nin]))
            seen[b * outs: b * outs + nout] = True
        rest = got[~seen]
        return ok and bool(np.isnan(rest.view(np.float32)).all()), "rows" if not ok else "gaps written"

    def ovsave_real(self, c):
        taps = taps_of(self.O, c)
        x = case_input(self.O, c)
        plan = self.ovsave_plan(c)
        want = self.ovsave_real_ref.overlap_save_real(x, taps, c["N"])
        if plan.nout(c["n"]) != len(want) or plan.is_fused != (c["N"] == 2048):
            return False, ("nout / is_fused", plan.nout(c["n"]), len(want))
        out = self.nans(len(want) + 8)
        got = plan(self.dev(x), out=out).cpu().numpy()
        return same_nan(got, want) and self.still_nan(out[len(want):]), "values"

    def pspec_common(self, c, real, dx, want, aligned=None):
        """the entry call itself on a NaN-filled output with a guard behind it, and the integration of ready spectra where it applies"""
        plan = self.pspec_plan(c, real)
        plan.set_split(c["mode"])
        if plan.nrows(c["n"]) != len(want) or plan.is_fused != c["route"]["fused"]:
            return False, ("nrows / is_fused", plan.nrows(c["n"]), len(want))
        out = self.nans(want.size + 8)
        got = plan(dx, out=out).cpu().numpy()
        if not (same_nan(got, want) and self.still_nan(out[want.size:])):
            return False, "entry"
        if c["window"] == "none" and c["step"] == c["N"] and len(want):
            ntr = len(want) * c["K"]
            src = (dx if aligned is None else aligned)[: ntr * c["N"]]
            X = (self.plan(("Fftr", c["N"], False), lambda: self.R.Fftr(c["N"])) if real else self.plan(("Fft", c["N"]), lambda: self.R.Fft(c["N"])))(src)
            if not same_nan(self.spectra_route(plan, X, want.shape[1]).cpu().numpy(), want):
                return False, "spectra"
        return True, ""

    def spectra_route(self, plan, X, bins):
        """plan.spectra on the ready spectra X, handed over with a row of NaN before and behind them: a row index that strays by one reads those"""
        t = self.t
        words = self.nans(2 * (X.numel() + 2 * bins))
        buf = t.view_as_complex(words.view(-1, 2))
        mid = buf[bins: bins + X.numel()]
        mid.copy_(X)
        return plan.spectra(mid)

    def pspec(self, c):
        x = case_input(self.O, c)
        want = self.pspec_ref.power_spectrum(x, c["N"], c["K"], c["step"], window_of(self.O, c))
        return self.pspec_common(c, False, self.dev(x), want)

    def pspec_u8(self, c):
        raw = case_input(self.O, c)
        x = samples_of(self.O, raw)
        want = self.pspec_ref.power_spectrum(x, c["N"], c["K"], c["step"], window_of(self.O, c))
        rd = self.dev(raw, c["base"])
        plan = self.pspec_plan(c, False)
        plan.set_split(c["mode"])

        def u8():
            out = self.nans(want.size + 8)
            got = plan.u8(rd, out=out).cpu().numpy()
            return same_nan(got, want) and self.still_nan(out[want.size:])

        def two_calls():   # redio_data_to_samples, then the cf32 entry on the same plan object
            xs = self.R.bitfount.data_to_samples(self.dev(raw)) if c["n"] else self.dev(np.zeros(0, np.complex64))
            return same_nan(plan(xs).cpu().numpy(), want)

        for name, f in ([("u8", u8), ("two calls", two_calls)] if c["u8_first"] else [("two calls", two_calls), ("u8", u8)]):
            if not f():
                return False, name
        return True, ""

    def pspec_real(self, c):
        x = case_input(self.O, c)
        want = self.pspec_real_ref.power_spectrum(x, c["N"], c["K"], c["step"], window_of(self.O, c))
        dx = self.dev(x, c["base"])
        assert dx.data_ptr() % 8 == c["base"]
        return self.pspec_common(c, True, dx, want, aligned=self.dev(x) if c["base"] else None)

    def streams(self, c):
        t, kind, n = self.t, c["kind"], c["rows"]
        x = case_input(self.O, c)
        if kind == "ovsave_real":
            plan = self.ovsave_plan(c)
            want = self.ovsave_real_ref.overlap_save_real(x, taps_of(self.O, c), c["N"])
        elif kind == "pspec_real":
            plan = self.pspec_plan(c, True)
            want = self.pspec_real_ref.power_spectrum(x, c["N"], c["K"], c["step"], window_of(self.O, c))
        else:
            plan = self.pspec_plan(c, False)
            want = self.pspec_ref.power_spectrum(samples_of(self.O, x) if kind == "pspec_u8" else x, c["N"], c["K"], c["step"], window_of(self.O, c))
        want = np.asarray(want, np.float32).reshape(-1)
        per = 2 if kind == "pspec_u8" else 1     # elements of the device view per sample
        dx = self.dev(x)
        st = self.R.Stream(plan, u8=kind == "pspec_u8")
        cuts = np.concatenate([[0], np.cumsum(c["pieces"])]).astype(np.int64)
        for which, cuts in (("first pass", cuts), ("after reset", None if c["again"] is None else np.array([0] + c["again"] + [n], np.int64))):
            if cuts is None:
                break
            if which == "after reset":
                st.reset()
            outs = [st(dx[per * int(lo): per * int(hi)]).clone() for lo, hi in zip(cuts[:-1], cuts[1:])]
            got = t.cat(outs).cpu().numpy() if outs else np.zeros(0, np.float32)
            if not same_nan(got, want):
                return False, which
        return True, ""

    # -- the polyphase spectrometer --
    def pfb_plan(self, c):
        key = ("PolyphaseSpectrum", c["M"], c["P"], c["K"], c["fir_fused"], c["taps"], c["tseed"] if c["taps"] == "synth" else 0, c["block"])
        return self.plan(key, lambda: self.R.PolyphaseSpectrum(pfb_taps_of(self.O, c), c["M"], c["P"], c["K"], fused=c["fir_fused"], one_kernel=c["block"]))

    def pfb_pspec(self, c):
        ref, M, P, K, ff = self.pfb_pspec_ref, c["M"], c["P"], c["K"], c["fir_fused"]
        h = pfb_taps_of(self.O, c)
        x, raw = pfb_input(self.O, c, False), pfb_input(self.O, c, True)
        want, want8 = ref.spectrum(x, h, M, P, K, ff), ref.spectrum_u8(raw, h, M, P, K, ff)
        T = c["n"] // M
        rows = 0 if T < P + K - 1 else (T - P + 1) // K     # redio.h: nrows = (T - P + 1) / K, 0 when T < P + K - 1
        plan = self.pfb_plan(c)
        plan.set_split(c["mode"])
        if not (plan.nrows(c["n"]) == rows == len(want) == len(want8) == c["rows"]) or plan.is_fused != c["route"]["fused"]:
            return False, ("nrows / is_fused", plan.nrows(c["n"]), rows, len(want), plan.is_fused)
        if plan.route != c["route"]["route"]:
            return False, ("route", plan.route)
        dx = self.dev(x, c["cbase"])
        assert dx.data_ptr() % 16 == c["cbase"]
        out = self.nans(want.size + 8)
        got = plan(dx, out=out).cpu().numpy()
        if not (same_nan(got, want) and self.still_nan(out[want.size:])):
            return False, "cf32 entry"
        rd = self.dev(raw, c["base"])

        def from_bytes():
            out = self.nans(want8.size + 8)
            got = plan.from_bytes(rd, out=out).cpu().numpy()
            return same_nan(got, want8) and self.still_nan(out[want8.size:])

        def two_calls():   # redio_data_to_samples, then the cf32 entry on the same plan object
            xs = self.R.bitfount.data_to_samples(self.dev(raw)) if c["n"] else self.dev(np.zeros(0, np.complex64))
            return same_nan(plan(xs).cpu().numpy(), want8)

        for name, f in ([("from_bytes", from_bytes), ("two calls", two_calls)] if c["u8_first"] else [("two calls", two_calls), ("from_bytes", from_bytes)]):
            if not f():
                return False, name
        if rows:   # the definition: redio_pfb_enqueue, then redio_pspec_enqueue_spectra of a (nfft = M, integrate = K) plan
            chan = self.plan(("Channelizer", M, P, ff, c["taps"], c["tseed"] if c["taps"] == "synth" else 0), lambda: self.R.Channelizer(h, M, P, ff))
            X = chan(self.dev(x))[: rows * K].reshape(-1)
            integ = self.pspec_plan({"N": M, "K": K, "step": M, "window": "none"}, False)
            if not same_nan(self.spectra_route(integ, X, M).cpu().numpy(), want):
                return False, "composition"
        return True, ""

    def pfb_streams(self, c):
        t, ref, M, P, K, u8, n = self.t, self.pfb_pspec_ref, c["M"], c["P"], c["K"], c["u8"], c["rows"]
        H = K * M
        h = pfb_taps_of(self.O, c)
        x = pfb_input(self.O, c, u8)
        want = (ref.spectrum_u8 if u8 else ref.spectrum)(x, h, M, P, K, c["fir_fused"]).reshape(-1)
        per = 2 if u8 else 1     # elements of the device view per sample
        dx = self.dev(x)
        plan = self.pfb_plan(c)
        plan.set_split(0)   # a cached plan may come from a pfb_pspec case that named its mode
        if plan.route != c["route"]["route"] or plan.is_fused != c["route"]["fused"]:
            return False, ("route / is_fused", plan.route, plan.is_fused)
        st = self.R.Stream(plan, u8=u8)
        cuts = np.concatenate([[0], np.cumsum(c["pieces"])]).astype(np.int64)
        for which, cuts in (("first pass", cuts), ("after reset", None if c["again"] is None else np.array([0] + c["again"] + [n], np.int64))):
            if cuts is None:
                break
            if which == "after reset":
                st.reset()
                if st.pending != 0:
                    return False, "pending after reset"
            outs, made = [], 0
            for lo, hi in zip(cuts[:-1], cuts[1:]):
                lo, hi = int(lo), int(hi)
                expect = ref.nrows(hi, M, P, K) - made
                if st.nout(hi - lo) != expect * M:
                    return False, (which, "nout", lo, hi)
                y = st(dx[per * lo: per * hi])
                if y.numel() != expect * M:
                    return False, (which, "count", lo, hi)
                outs.append(y.clone())
                made += expect
                if st.pending != hi - made * H:
                    return False, (which, "pending", lo, hi)
            got = t.cat(outs).cpu().numpy() if outs else np.zeros(0, np.float32)
            if not same_nan(got, want):
                return False, which
        return True, ""

    def run(self, c):
        try:
            ok, why = getattr(self, c["family"])(c)
        except (AssertionError, self.R.RedioError) as e:   # a refused valid call or a host-side size check: a finding like any other
            ok, why = False, repr(e)
        t = self.t
        t.cuda.synchronize()
        brief = {k: v for k, v in c.items() if k != "route"}
        check(c["family"], ok, (why, json.dumps(brief)))
        if "route" in c["route"]:   # the polyphase spectrometer's cases: a count per family and route
            per_route = f"{c['family']} route {c['route']['route']}"
            runs[per_route] = runs.get(per_route, 0) + 1


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
    print("runs", runs, "failures", fails)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main())
