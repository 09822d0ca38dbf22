"""redio_pfb_pspec_* above the floor of its launch geometry.  pfbspec_units_per_wave (libredio_amd/csrc/pfb_pspec_core.h) gives a
wavefront max(ceil(nunits / 2048), least) consecutive units -- output rows, or in segment mode segments -- with least = ceil(64 / K)
rows or 4 segments.  Up to about 2^23 samples every call sits on `least`; the headline sizes do not.  These calls of 4.4 to 8.5 M samples
give a wave ceil(nunits / 2048) units: the last wave is shorter, and in segment mode a run of an odd number of segments starts in the
middle of an output row.  Auto mode is called either side of its threshold of 1024 * ceil(64 / K) output rows.  Bit for bit against
the restatement (tests/pfb_pspec_ref.py) of the whole input, from cf32 samples and -- the byte kernel requests its rows later -- from
u8 I/Q bytes at byte offset 2.  The figures of the table are asserted from a restatement of the launcher's arithmetic, so that a change
of its constants fails here instead of leaving these shapes on the floor."""
import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F5E
M = 64
SEG = 16            # PSPEC_SEG
WAVES = 8 * 256     # the waves pfbspec_units_per_wave aims at
SPLIT_WAVES = 1024  # PFBSPEC_SPLIT_WAVES
AUTO, ROWS, SEGMENTS = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def units_per_wave(nunits, K, split):
    """pfbspec_units_per_wave: (units a wave owns, its floor)"""
    per_unit = SEG if split else K
    least = -(-4 * 16 // per_unit)
    return max(-(-nunits // WAVES), least), least


def geometry(mode, K, rows):
    """(split, units, units per wave, floor) of a call of `rows` output rows on a fused plan"""
    S = -(-K // SEG)
    split = S >= 2 and (mode == SEGMENTS or (mode == AUTO and rows < SPLIT_WAVES * units_per_wave(1, K, False)[0]))
    units = rows * S if split else rows
    return (split, units) + units_per_wave(units, K, split)


# mode, P, K, output rows, from bytes, (split, units, units per wave) as the launcher must choose them
ABOVE = [
    (ROWS, 16, 64, 2049, False, (False, 2049, 2)),       # 1025 waves, the last one short
    (ROWS, 16, 64, 2049, True, (False, 2049, 2)),
    (ROWS, 4, 1, 131073, False, (False, 131073, 65)),    # floor 64
    (ROWS, 8, 5, 26631, False, (False, 26631, 14)),      # floor 13
    (SEGMENTS, 8, 17, 4097, False, (True, 8194, 5)),     # S = 2 and runs of 5: every other wave starts in the middle of a row
    (SEGMENTS, 8, 17, 4097, True, (True, 8194, 5)),
    (SEGMENTS, 16, 40, 2731, False, (True, 8193, 5)),    # S = 3
]
# auto, either side of 1024 * ceil(64 / K) output rows: segments below, whole rows from there on
THRESHOLD = [(8, 17, 4095, False), (8, 17, 4096, False), (8, 17, 4095, True), (8, 17, 4096, True), (16, 40, 2047, False), (16, 40, 2048, False)]


def run(gpu, redio, oracle, mode, P, K, rows, u8):
    """`rows` output rows, K - 1 channelizer rows of a dropped one and 3 stray samples, on a NaN-filled output with a guard behind it"""
    n = M * (rows * K + P - 1) + M * (K - 1) + 3
    assert 4_400_000 <= n < 8_600_000
    h = oracle.lpf_corrected(M * P, 0.45 / M) if P == 16 else oracle.synth_f32(9, P, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    assert plan.is_fused and plan.nrows(n) == rows
    plan.set_split(mode)
    out = gpu.full((rows * M + M,), float("nan"), dtype=gpu.float32, device="cuda")
    if u8:
        raw = np.random.default_rng(SEED + K).integers(0, 256, 2 * n + 2, dtype=np.uint8)
        big = gpu.from_numpy(raw).cuda()
        assert big.data_ptr() % 16 == 0
        got = plan.from_bytes(big[2:], out=out)
        want = ref.spectrum_u8(raw[2:], h, M, P, K, True)
    else:
        x = redio.synth_iq(SEED, K, n)
        got = plan(x, out=out)
        want = ref.spectrum(x.cpu().numpy(), h, M, P, K, True)
    assert want.shape == (rows, M) and not np.isnan(want).any()
    got = got.cpu().numpy()
    bad = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    assert got.shape == want.shape and not len(bad), (len(bad), bad[:8])
    assert bool(out[rows * M:].isnan().all())


@pytest.mark.parametrize("mode,P,K,rows,u8,stated", ABOVE)
def test_units_per_wave_above_the_floor(gpu, redio, oracle, mode, P, K, rows, u8, stated):
    split, units, upw, floor = geometry(mode, K, rows)
    assert (split, units, upw) == stated and upw > floor, "this shape no longer runs above the launcher's floor"
    assert units % upw, "the last wave is no longer a short one"
    if split:
        assert upw % -(-K // SEG), "no wave starts in the middle of an output row any more"
    run(gpu, redio, oracle, mode, P, K, rows, u8)


@pytest.mark.parametrize("P,K,rows,u8", THRESHOLD)
def test_auto_either_side_of_its_threshold(gpu, redio, oracle, P, K, rows, u8):
    edge = SPLIT_WAVES * -(-64 // K)
    assert rows in (edge - 1, edge), "these row counts are no longer the two sides of auto's threshold"
    assert geometry(AUTO, K, rows)[0] == (rows < edge)
    run(gpu, redio, oracle, AUTO, P, K, rows, u8)
