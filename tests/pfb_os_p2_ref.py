"""What the tests of the oversampled channelizer's workgroup kernel (redio_pfb_os_* with REDIO_PFB_OS_BLOCK, route 2) share: the route
rule of tests/pfb_os_ref.py extended by the flag, the kernel's shape constants and launch geometry restated
(libredio_amd/csrc/pfb_os_p2_core.h), the image's leaf order (fft_p2.h), the row counts the cases use, and the inputs and the wanted
rows -- computed once, shared, never written to."""
import functools

import numpy as np

import pfb_os_ref as ref

SEED = 0x5EED0B52
CHANNELS = (32, 128, 256, 512, 1024)
TAPS = (4, 8, 16)
# 1024 channels x 16 taps has no workgroup form: its register windows only fit with spills; it stays on route 0
LEFT_OUT = ((1024, 16),)
ALL_SHAPES = [(M, P) for M in CHANNELS for P in TAPS]
SHAPES = [s for s in ALL_SHAPES if s not in LEFT_OUT]


def route(M, P, H, block):
    """pfb_os_ref.route with the flag: 2 the workgroup kernel, 1 the 64-channel wave kernel, 0 two passes"""
    if ref.route(M, P, H) == 1:
        return 1
    if block and M in CHANNELS and P in TAPS and 2 * H == M and (M, P) not in LEFT_OUT:
        return 2
    return 0


def shape_consts(M):
    """(G, TR): streams per workgroup, rows per stream and iteration (pfb_p2_kernel's, the same in both load forms)"""
    return (1, 4096 // M) if M >= 256 else (256 // M, 16)


def rows_per_stream(rows, cus, M):
    G, TR = shape_consts(M)
    rps = -(-rows // (4 * cus * G))
    rps = -(-rps // TR) * TR
    return max(rps, 64)


def leaf_pos(n, M):
    """FftP2<log2 M>::leaf_pos: the top bit is the radix-2 digit, the base-4 digits reverse onto M / 4, M / 16, ..."""
    L = M.bit_length() - 1
    L4 = L // 2
    pos = n >> (2 * L4) if L & 1 else 0
    for i in range(L4):
        pos += ((n >> (2 * i)) & 3) * (M >> (2 * i + 2))
    return pos


def rows_list(M):
    """none, one, around an iteration, around a stream's smallest run (64), past one workgroup, and past three with a short end"""
    G, TR = shape_consts(M)
    return sorted({0, 1, TR - 1, TR, TR + 1, 63, 64, 65, 64 * G + 1, 3 * 64 * G + 5})


def n_in(M, P, rows):
    return M * P + (M // 2) * (rows - 1) if rows else M * P - 1


@functools.lru_cache(maxsize=None)
def case(M, P, fused):
    """input (with M / 2 - 1 samples behind the last row's window: never read), prototype and the ref's branch sums for the largest
    row count of rows_list(M)"""
    import oracle
    top = max(rows_list(M))
    x = oracle.synth_iq(SEED, 64 * M + P, n_in(M, P, top) + M // 2 - 1)
    h = oracle.synth_f32(3, M * P, M * P)
    u = ref.branch_sums(x, h, M, P, M // 2, fused)
    assert u.shape == (top, M)
    for a in (x, h, u):
        a.setflags(write=False)
    return x, h, u


@functools.lru_cache(maxsize=None)
def want_rotated(M, P, fused, fpar):
    """v_r for a first_row of parity fpar (at hop M / 2 the shift is M / 2 for odd F + r); row r of a shorter call is row r of this"""
    _, _, u = case(M, P, fused)
    v = ref.roll_rows(u, M, M // 2, fpar)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def want_rows(M, P, fused, fpar):
    import oracle
    v = want_rotated(M, P, fused, fpar)
    w = oracle.fft(np.ascontiguousarray(v.reshape(-1)), M, inverse=False).reshape(-1, M)
    w.setflags(write=False)
    return w
