"""tests/runs_ref.py -- the references that tests/test_gpu_runs_scans.py trusts -- against the restatements in oracle/, on the CPU."""
import numpy as np
import pytest

import runs_ref as ref

TIES = [(1 << 24) + 1, (1 << 24) + 3, (1 << 40) + (1 << 16), (1 << 40) + (1 << 16) + 1, (1 << 53) + 1, (1 << 54) + (1 << 30) + 1,
        1 << 63, (1 << 63) + (1 << 39), (1 << 63) + (1 << 39) + 1, (1 << 64) - 1]
DOUBLE_ROUNDED = [(1 << 54) + (1 << 30) + 1, (1 << 63) + (1 << 39) + 1]  # np.float32(int) goes through double and lands one ulp low


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def _stream(rng, kind, n):
    if kind == "binary":
        return np.repeat(rng.integers(0, 2, n), rng.integers(1, 40, n)).astype(np.uint8)[:n]
    if kind == "bytes":
        return np.repeat(rng.integers(0, 256, n), rng.integers(1, 4, n)).astype(np.uint8)[:n]
    if kind == "noise":
        return rng.integers(0, 256, n).astype(np.uint8)
    return np.full(n, rng.integers(0, 256), np.uint8)  # constant


@pytest.mark.parametrize("seed", range(40))
def test_rle_np_is_oracle_rle_on_cut_streams(oracle, seed):
    rng = np.random.default_rng(seed)
    kind = ("binary", "bytes", "noise", "constant")[seed % 4]
    x = _stream(rng, kind, int(rng.integers(1, 3000)))
    if seed % 5 == 0 and len(x) >= 8:       # 255 -> 0 and back, and a constant stretch in the middle
        x[len(x) // 3:len(x) // 3 + 4] = [255, 0, 255, 0]
        x[len(x) // 2:len(x) // 2 + 300] = 7
    cuts = set(rng.integers(0, len(x) + 1, int(rng.integers(0, 12))).tolist()) | {0, len(x)}
    if len(x) > 2:
        cuts |= {1, len(x) - 1}              # single-element calls
    cuts = sorted(cuts) + [len(x)]           # and an empty one at the end
    o, st = oracle.Rle(), ref.RleState()
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        v, c = ref.rle_np(x[lo:hi], st)
        want = o.feed(x[lo:hi])
        assert v.dtype == np.uint8 and c.dtype == np.uint64
        assert list(zip(v.tolist(), c.tolist())) == want, (lo, hi)
        assert (st.have_prev, st.prev, st.i) == (o.x is not None, o.x if o.x is not None else 0, o.i)


def test_rle_np_constant_calls_carry_the_open_run(oracle):
    o, st = oracle.Rle(), ref.RleState()
    for call in ([5] * 10, [5], [5] * 300, [6], [6] * 2, [255], [0], [0] * 17, [255]):
        v, c = ref.rle_np(np.array(call, np.uint8), st)
        assert list(zip(v.tolist(), c.tolist())) == o.feed(call)
    assert (st.prev, st.i) == (255, 1)


def test_u64_to_f32_rne_is_the_single_rounding_cast():
    rng = np.random.default_rng(1)
    rnd = rng.integers(0, 1 << 64, 20000, dtype=np.uint64)
    rnd[:4000] >>= rng.integers(0, 64, 4000).astype(np.uint64)           # every magnitude, not only the top binades
    cts = np.concatenate((np.array(TIES + [0, 1, (1 << 24) - 1, 1 << 24], np.uint64), rnd))
    assert np.array_equal(bits(ref.u64_to_f32_rne(cts)), bits(cts.astype(np.float32)))
    for ct in TIES:
        assert bits(ref.u64_to_f32_rne(ct)) == bits(np.array(ct, np.uint64).astype(np.float32))
    # the ties go to even, the values one above a tie go up
    assert float(ref.u64_to_f32_rne((1 << 24) + 1)) == float(1 << 24)
    assert float(ref.u64_to_f32_rne((1 << 24) + 3)) == float((1 << 24) + 4)
    assert float(ref.u64_to_f32_rne((1 << 63) + (1 << 39))) == float(1 << 63)
    assert float(ref.u64_to_f32_rne((1 << 63) + (1 << 39) + 1)) == float((1 << 63) + (1 << 40))
    assert float(ref.u64_to_f32_rne((1 << 54) + (1 << 30) + 1)) == float((1 << 54) + (1 << 31))
    assert float(ref.u64_to_f32_rne((1 << 64) - 1)) == 2.0 ** 64
    for ct in DOUBLE_ROUNDED:                                              # what oracle.dle did before it converted with one rounding
        assert bits(np.float32(ct)) != bits(ref.u64_to_f32_rne(ct))


@pytest.mark.parametrize("s_rate", [256000, 1, 16777217, 48000])
def test_dle_ref_is_oracle_dle(oracle, s_rate):
    rng = np.random.default_rng(2)
    cts = TIES + [0, 1, 51, 512, 1000] + rng.integers(0, 1 << 64, 2000, dtype=np.uint64).tolist()
    got = ref.dle_ref(np.array(cts, np.uint64), s_rate)
    want = oracle.dle([(1, ct) for ct in cts], s_rate)
    assert got.dtype == np.float32
    assert np.array_equal(bits(got), bits([w[1] for w in want]))


def test_dld_counts_ref_saturates_like_the_cast():
    f = np.float32
    sub = np.frombuffer(np.uint32(1).tobytes(), np.float32)[0]
    dur = np.array([np.nan, -1.0, -0.0, 0.0, sub, np.inf, 1e30, 0.5, np.nextafter(f(1.0), f(0)), 1.0, 2.0 ** 40, 2.0 ** 63, 2.0 ** 64,
                    np.nextafter(f(2.0 ** 64), f(0))], np.float32)
    got = ref.dld_counts_ref(dur, 1.0).tolist()
    assert got == [0, 0, 0, 0, 0, ref.U64_MAX, ref.U64_MAX, 0, 0, 1, 1 << 40, 1 << 63, ref.U64_MAX, (1 << 64) - (1 << 40)]


def test_dld_counts_ref_is_oracle_dld(oracle):
    rng = np.random.default_rng(3)
    for rate in (256000.0, 48000.0):
        dur = np.concatenate(((rng.random(300) * 0.004).astype(np.float32), ref.dle_ref(np.arange(1, 200), int(rate))))
        vals = rng.integers(0, 256, len(dur)).astype(np.uint8)
        want = oracle.dld(list(zip(vals.tolist(), dur.tolist())), rate)
        assert ref.rld_ref(vals, ref.dld_counts_ref(dur, rate)).tolist() == want


def test_rld_ref_is_oracle_rld(oracle):
    rng = np.random.default_rng(4)
    vals = rng.integers(0, 256, 500).astype(np.uint8)
    counts = rng.choice([0, 1, 2, 255, 256, 257], 500).astype(np.uint64)
    assert ref.rld_ref(vals, counts).tolist() == oracle.rld(list(zip(vals.tolist(), counts.tolist())))
    assert ref.rld_ref(vals[:3], np.zeros(3, np.uint64)).size == 0


@pytest.mark.parametrize("widths", [[4, 8, 4, 12, 8], [64], [63, 1], [0, 64, 0], [1] * 64, [32, 32], [0], [1], [7, 0, 3]])
def test_binconv_ref_is_oracle_eat_on_binary_digits(oracle, widths):
    rng = np.random.default_rng(len(widths))
    bits01 = rng.integers(0, 2, (40, sum(widths) + 3)).astype(np.uint8)
    bits01[0], bits01[1] = 0, 1
    got = ref.binconv_ref(bits01, widths)
    assert got.dtype == np.uint64 and got.shape == (40, len(widths))
    assert got.tolist() == [oracle.eat(b[:sum(widths)], widths) for b in bits01]
    if 64 in widths:
        assert got[1, widths.index(64)] == ref.U64_MAX


def test_binconv_ref_multiplies_digits_beyond_one(oracle):
    # the reference multiplies the digit (kpn.rs:112); a digit of 2 or 255 is neither `& 1` nor `!= 0`
    rng = np.random.default_rng(5)
    widths = [48, 3, 13]
    digits = rng.integers(0, 256, (30, 64)).astype(np.uint8)
    got = ref.binconv_ref(digits, widths)
    assert got.tolist() == [oracle.eat(b, widths) for b in digits]
    assert ref.binconv_ref(np.array([[2, 255, 1]], np.uint8), [3]).tolist() == [[2 * 4 + 255 * 2 + 1]]
