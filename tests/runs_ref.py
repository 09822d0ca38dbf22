"""Plain references of the run-length / bit-field stage (kpn::rle, dle, dld, rld, binconv; src/kpn/src/kpn.rs) in numpy and Python
integers: the checkers of runs.hip at sizes where oracle.Rle's per-element loop is unusable (10^8 bytes) and at counts where a
conversion through double is inexact (above 2^53).  tests/test_runs_ref_cpu.py checks them against oracle/ where both apply."""
import numpy as np

U64_MAX = (1 << 64) - 1


class RleState:
    """what kpn::rle carries between calls (kpn.rs:18-19): whether a sample ever arrived, the last value, the open run's length"""
    __slots__ = ("have_prev", "prev", "i")

    def __init__(self, have_prev=False, prev=0, i=0):
        self.have_prev, self.prev, self.i = bool(have_prev), int(prev), int(i)

    def copy(self):
        return RleState(self.have_prev, self.prev, self.i)


def rle_np(x, state):
    """kpn::rle (kpn.rs:17-29) over one call's values: a run is emitted when the value changes, the first sample ever only seeds, the open
    run is never flushed.  Updates state in place; returns (vals u8, counts u64) of the runs this call completed."""
    x = np.ascontiguousarray(x, dtype=np.uint8)
    n = len(x)
    if n == 0:
        return np.empty(0, np.uint8), np.empty(0, np.uint64)
    before0 = state.prev if state.have_prev else int(x[0])  # the first sample ever differs from nothing
    carried = state.i if state.have_prev else 0
    p = np.flatnonzero(x[1:] != x[:-1]) + 1                  # positions whose value differs from the one in front
    if int(x[0]) != before0:
        p = np.concatenate(([0], p))
    p = p.astype(np.int64)
    if len(p):
        vals = np.where(p > 0, x[np.maximum(p - 1, 0)], np.uint8(before0)).astype(np.uint8)  # the value of the run that the change ends
        counts = np.diff(p, prepend=0).astype(np.uint64)
        counts[0] = np.uint64(int(p[0]) + carried)
        state.i = n - int(p[-1])
    else:
        vals, counts = np.empty(0, np.uint8), np.empty(0, np.uint64)
        state.i = carried + n
    state.have_prev, state.prev = True, int(x[-1])
    return vals, counts


def _u64_to_f32_bits(ct):
    ct = int(ct)
    assert 0 <= ct <= U64_MAX
    if ct == 0:
        return 0
    e = ct.bit_length() - 1
    if e <= 23:
        m = ct << (23 - e)
    else:
        sh = e - 23
        m, rem, half = ct >> sh, ct & ((1 << sh) - 1), 1 << (sh - 1)
        if rem > half or (rem == half and (m & 1)):
            m += 1
        if m == 1 << 24:      # the rounding carried into the next binade
            m, e = m >> 1, e + 1
    return ((e + 127) << 23) | (m & 0x7FFFFF)


def u64_to_f32_rne(ct):
    """`ct as f32` of a u64 (kpn.rs:35): ONE round-to-nearest-even, in integer arithmetic.  A scalar gives np.float32, anything else an
    array of the same shape."""
    if np.ndim(ct) == 0:
        return np.array([_u64_to_f32_bits(ct)], np.uint32).view(np.float32)[0]
    a = np.asarray(ct)
    flat = [_u64_to_f32_bits(v) for v in a.reshape(-1).tolist()]
    return np.array(flat, np.uint32).view(np.float32).reshape(a.shape)


def dle_ref(counts, s_rate):
    """kpn::dle (kpn.rs:32-38): ct as f32 / s_rate as f32, both conversions from unsigned 64-bit integers"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return (u64_to_f32_rne(counts) / u64_to_f32_rne(int(s_rate))).astype(np.float32)


def dld_counts_ref(dur_f32, s_rate_f32):
    """(dur * s_rate) as usize (kpn.rs:44): the product in f32, then Rust's saturating cast -- NaN and everything <= 0 (-0.0 too) give
    0, 2^64 and beyond give 2^64 - 1, the rest truncates"""
    with np.errstate(over="ignore", invalid="ignore"):
        v = (np.atleast_1d(np.asarray(dur_f32, np.float32)) * np.float32(s_rate_f32)).astype(np.float32)
        out = np.zeros(v.shape, np.uint64)
        big = v >= np.float32(2.0 ** 64)
        mid = (v > 0) & ~big
        out[big] = np.uint64(U64_MAX)
        out[mid] = np.array([int(t) for t in v[mid].astype(np.float64).tolist()], dtype=np.uint64)  # every f32 is an exact double; int() truncates exactly
    return out


def rld_ref(vals, counts):
    """kpn::rld (kpn.rs:50-56)"""
    counts = np.asarray(counts, np.uint64)
    assert counts.size == 0 or int(counts.max()) < 1 << 62
    return np.repeat(np.asarray(vals, np.uint8), counts.astype(np.int64))


def binconv_ref(bits, widths):
    """kpn::binconv (kpn.rs:295-299) = eat (:116-124) of b2d (:111-113) per message: field f of width w is sum(2**(w-i-1) * digit_i) over
    its digits, MSB first, in Python integers.  bits is [nmsg, nbits]; returns u64 [nmsg, len(widths)] (the sums must fit)."""
    bits = np.asarray(bits)
    nmsg, nbits = bits.shape
    assert sum(widths) <= nbits
    out = np.zeros((nmsg, len(widths)), np.uint64)
    start = 0
    for f, w in enumerate(widths):
        acc = np.array([0] * nmsg, dtype=object)
        for i in range(w):
            acc = acc + 2 ** (w - i - 1) * bits[:, start + i].astype(object)
        assert all(0 <= int(a) <= U64_MAX for a in acc)
        out[:, f] = np.array([int(a) for a in acc], dtype=np.uint64)
        start += w
    return out
