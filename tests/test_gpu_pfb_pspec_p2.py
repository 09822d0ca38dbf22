"""redio_pfb_pspec_* with REDIO_PFB_PSPEC_BLOCK on the GPU: the workgroup kernel (route 2) of the 15 one-kernel channelizer shapes bit
for bit against the restatement (tests/pfb_pspec_ref.py: oracle.pfb_channelizer, then pspec_ref.spectra) and against the unflagged
plan, from cf32 samples at 16- and 8-byte aligned bases and from u8 I/Q bytes at byte offsets 0 and 2, by rows and by segments, on
NaN-filled outputs with a guard behind them; inputs that end where a guard region begins; and the amplitude ladder."""
import numpy as np
import pytest

import pfb_pspec_ref as ref
import spectrum_ladder as sl

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F60
SHAPES = [(M, P) for M in (32, 128, 256, 512, 1024) for P in (4, 8, 16)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def test_routes(gpu, redio, oracle):
    PS = redio.PolyphaseSpectrum
    assert (PS.GENERIC, PS.WAVE, PS.BLOCK) == (0, 1, 2)
    for M, P in SHAPES:
        plan = PS(oracle.synth_f32(9, 0, M * P), M, P, 5, one_kernel=True)
        assert plan.route == PS.BLOCK and not plan.is_fused, (M, P)
    h = oracle.synth_f32(9, 0, 128 * 8)
    assert PS(h, 128, 8, 5).route == PS.GENERIC
    plan = PS(oracle.synth_f32(9, 0, 64 * 16), 64, 16, 5, one_kernel=True)
    assert plan.route == PS.WAVE and plan.is_fused
    plan = PS(oracle.synth_f32(9, 0, 100 * 5), 100, 5, 5, one_kernel=True)
    assert plan.route == PS.GENERIC and not plan.is_fused


def call(gpu, plan, fn, d, want, what):
    """one call on a NaN-filled output with a row of guard words behind it"""
    M = plan.nchan
    out = gpu.full((want.size + M,), float("nan"), dtype=gpu.float32, device="cuda")
    got = fn(d, out=out)
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got.cpu().numpy()), bits(want)), what
    assert bool(out[want.size:].isnan().all()), what  # nothing behind the rows, and nothing at all without a row
    return got


def check(gpu, redio, oracle, M, P, K, fused):
    h = oracle.synth_f32(9, P, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K, fused=fused, one_kernel=True)
    base = redio.PolyphaseSpectrum(h, M, P, K, fused=fused)
    assert plan.route == plan.BLOCK and not plan.is_fused and base.route == base.GENERIC
    modes = (plan.ROWS, plan.SEGMENTS) if K > 16 else (plan.AUTO,)
    for T in (P + K - 2, P + K - 1, 3 * K + P - 1 + (K - 1)):
        n = M * T + 3
        x = oracle.synth_iq(SEED + M, T, n)
        want = ref.spectrum(x, h, M, P, K, fused)
        assert want.shape == (max(T - P + 1, 0) // K, M) and plan.nrows(n) == len(want) and not np.isnan(want).any()
        big = gpu.zeros(n + 1, dtype=gpu.complex64, device="cuda")
        assert big.data_ptr() % 16 == 0
        d16, d8 = big[:n], big[1:]  # the second: 8- but not 16-byte aligned, the 8-byte loads at 512 and 1024 channels
        raw = random_bytes(SEED + T + M, 2 * n + 2)
        rbig = gpu.from_numpy(raw).cuda()
        assert rbig.data_ptr() % 16 == 0
        want_u8 = {0: ref.spectrum_u8(raw[: 2 * n], h, M, P, K, fused), 2: ref.spectrum_u8(raw[2:], h, M, P, K, fused)}
        for mode in modes:
            plan.set_split(mode)
            d16.copy_(gpu.from_numpy(x))
            got = call(gpu, plan, plan, d16, want, (T, mode, "cf32 at 16"))
            if len(want):
                assert gpu.equal(got.view(gpu.int32), base(d16).view(gpu.int32)), (T, mode)
            d8.copy_(gpu.from_numpy(x))
            call(gpu, plan, plan, d8, want, (T, mode, "cf32 at 8"))
            for off, rd in ((0, rbig[: 2 * n]), (2, rbig[2:])):
                got = call(gpu, plan, plan.from_bytes, rd, want_u8[off], (T, mode, "bytes at", off))
                if len(want) and mode == modes[0]:
                    assert gpu.equal(got.view(gpu.int32), base.from_bytes(rd).view(gpu.int32)), (T, off)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("M,P", SHAPES)
def test_every_shape_bit_exact(gpu, redio, oracle, M, P, fused):
    check(gpu, redio, oracle, M, P, 17, fused)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("K", [1, 5, 16, 40])  # 17: above
@pytest.mark.parametrize("M,P", [(128, 8), (256, 16), (1024, 4)])
def test_every_integration_bit_exact(gpu, redio, oracle, M, P, K, fused):
    check(gpu, redio, oracle, M, P, K, fused)


@pytest.mark.parametrize("chrows", [17, 33, 200])
@pytest.mark.parametrize("M,P,K", [(32, 16, 3), (256, 8, 17), (1024, 4, 17)])
def test_streams_end_at_a_guard_region(gpu, redio, oracle, M, P, K, chrows):
    """the byte stream and the cf32 stream are views that end exactly where 4 KiB of 0xFF bytes or NaNs begin: rows past the end of
    the stream are never part of a result"""
    h = oracle.synth_f32(9, P, M * P)
    n = M * (chrows + P - 1)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK
    x = oracle.synth_iq(SEED, chrows, n)
    raw = random_bytes(SEED + chrows, 2 * n)
    want, want_u8 = ref.spectrum(x, h, M, P, K, True), ref.spectrum_u8(raw, h, M, P, K, True)
    big = gpu.full((n + 512,), float("nan"), dtype=gpu.complex64, device="cuda")
    big[:n] = gpu.from_numpy(x)
    rbig = gpu.full((2 * n + 4096,), 255, dtype=gpu.uint8, device="cuda")
    rbig[: 2 * n] = gpu.from_numpy(raw)
    for mode in (plan.ROWS, plan.SEGMENTS):
        plan.set_split(mode)
        got = plan(big[:n]).cpu().numpy()
        assert got.shape == want.shape == (chrows // K, M) and np.array_equal(bits(got), bits(want)), mode
        got = plan.from_bytes(rbig[: 2 * n]).cpu().numpy()
        assert got.shape == want_u8.shape and np.array_equal(bits(got), bits(want_u8)), mode


@pytest.mark.parametrize("M,P,K", [(32, 4, 17), (512, 8, 5), (1024, 16, 40)])
def test_nothing_behind_the_last_row_reaches_a_result(gpu, redio, oracle, M, P, K):
    """the call may read input rows up to nrows K + P - 2.  Behind them lie K - 1 rows of a dropped output row and 3 samples, here
    NaN, and then 4 KiB of NaN outside the call: no output is NaN, and all equal the restatement of the finite part"""
    h = oracle.synth_f32(9, P, M * P)
    nrows = 3
    keep = M * (nrows * K + P - 1)
    n = keep + M * (K - 1) + 3
    x = oracle.synth_iq(SEED, K, n)
    want = ref.spectrum(x[:keep], h, M, P, K, True)
    assert want.shape == (nrows, M)
    big = gpu.full((n + 512,), float("nan"), dtype=gpu.complex64, device="cuda")
    big[:keep] = gpu.from_numpy(x[:keep])
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK and plan.nrows(n) == nrows
    for mode in (plan.ROWS, plan.SEGMENTS):
        plan.set_split(mode)
        got = plan(big[:n]).cpu().numpy()
        assert not np.isnan(got).any() and np.array_equal(bits(got), bits(want)), mode


def test_range_ladder(gpu, redio, oracle):
    """tests/spectrum_ladder.py on a flagged 128 x 8, K = 17 plan: zeros, subnormals, overflow to inf, never NaN"""
    M, P, K, taps = shape = (128, 8, 17, "lpf")
    x, h, want = sl.case(oracle, "pfb", shape)
    c = sl.classes(want)
    assert c["nan"] == 0 and min(c["zero"], c["subnormal"], c["inf"], c["normal"]) > 0
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    assert plan.route == plan.BLOCK
    d = gpu.from_numpy(x).cuda()
    for mode in (plan.ROWS, plan.SEGMENTS):
        plan.set_split(mode)
        got = plan(d).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), mode
