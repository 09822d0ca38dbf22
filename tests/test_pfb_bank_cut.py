"""The chunk cut of the two-pass filterbank plans (libredio_amd/csrc/pfb_bank_cut.h: what pfb_bank.hip's reserve and enqueue use, and the
route-0 modes of tests/emu_pfb_os and tests/emu_pfb_os_synth), run on the CPU against a brute-force restatement: the passes of a call
cover every unit exactly once and in order, no pass holds more rows than reserve sized the scratch for, and every pass reads inside
the call's input."""
import ctypes as C

import pytest

SZ = C.c_size_t


def families(M, P, H):
    """(family, window, hop, unit_out, min_rows, row) of every plan this shape has, restated: family 0 the synthesis bank (rows M apart
    only), 1 the oversampled channelizer, 2 the oversampled synthesis bank"""
    L = -(-M * P // H)
    out = [(1, M * P, H, M, 1, M), (2, M * L, M, H, L, M)]
    if H == M:
        out.append((0, M * P, M, M, P, M))
    return out


def hops(M):
    odd = next(h for h in range(2, M) if M % h)  # the smallest hop that does not divide M
    return sorted({M, M // 2, 1, odd})


def brute(cut, asked, units):
    """one unit at a time: a pass of n units holds n + min_rows - 1 rows and takes units while they fit the chunk; what reserve has
    to size the scratch for is the largest pass that comes out"""
    window, hop, unit_out, min_rows, row = cut
    chunk = max(asked if asked else (64 << 20) // (row * 8), min_rows)
    passes, first, n = [], 0, 0
    for u in range(units):
        if n and (n + 1) + min_rows - 1 > chunk:
            passes.append((first, n))
            first, n = u, 0
        n += 1
    passes.append((first, n))
    passes = [(f, n, f * hop, n + min_rows - 1, f * unit_out) for f, n in passes]
    return chunk, max(p[3] for p in passes), passes


@pytest.mark.parametrize("M", [4, 5, 8, 12, 16, 33, 64])
def test_bank_cut_covers_every_unit_once_inside_scratch_and_input(emu, M):
    emu.emu_bank_units.restype = SZ
    emu.emu_bank_units.argtypes = [C.POINTER(SZ), SZ]
    emu.emu_bank_cut.argtypes = [C.POINTER(SZ), SZ, SZ, C.POINTER(SZ)]
    emu.emu_bank_pass.argtypes = [C.POINTER(SZ), SZ, SZ, SZ, C.POINTER(SZ)]
    emu.emu_bank_cut_of.argtypes = [C.c_int, SZ, SZ, SZ, C.POINTER(SZ)]
    cases = 0
    for P in range(1, 5):
        for H in hops(M):
            for name, *cut in families(M, P, H):
                window, hop, unit_out, min_rows, row = cut
                c5 = (SZ * 5)()
                emu.emu_bank_cut_of(name, M, P, H, c5)  # the entry the family's create function fills in
                assert list(c5) == cut, (name, M, P, H)
                for units in range(1, 41):
                    n_in = (units - 1) * hop + window  # what the call reads
                    assert emu.emu_bank_units(c5, n_in) == units and emu.emu_bank_units(c5, n_in - 1) == units - 1
                    assert emu.emu_bank_units(c5, n_in + hop - 1) == units
                    for asked in (0, min_rows, min_rows + 1, units + min_rows + 7, 1):  # 1: fewer rows than a pass needs count as min_rows
                        chunk, reserved, want = brute(cut, asked, units)
                        o3, o5 = (SZ * 3)(), (SZ * 5)()
                        emu.emu_bank_cut(c5, asked, units, o3)
                        assert tuple(o3) == (chunk, reserved, len(want)), (name, M, P, H, units, asked)
                        got = []
                        for i in range(o3[2]):
                            emu.emu_bank_pass(c5, asked, units, i, o5)
                            got.append(tuple(o5))
                        assert got == want, (name, M, P, H, units, asked)
                        # the properties themselves, on what the header answered
                        nxt = 0
                        for first, n, in_off, rows, out_off in got:
                            assert first == nxt and n >= 1  # every unit once, in order
                            nxt += n
                            assert rows <= reserved  # inside the reserved scratch
                            assert in_off + (n - 1) * hop + window <= n_in  # the pass's input ends inside the call's
                            assert out_off + n * unit_out <= units * unit_out
                        assert nxt == units
                        cases += 1
    assert cases >= 4 * 3 * 2 * 40 * 5
