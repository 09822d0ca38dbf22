"""redio_pfb_pspec_* on the GPU: the fused 64-channel kernel and the generic path bit for bit against the restatement
(tests/pfb_pspec_ref.py: oracle.pfb_channelizer, then pspec_ref.spectra), against the composition on the GPU (Channelizer, then
PowerSpectrum.spectra), from cf32 samples and from u8 I/Q bytes, in every split mode."""
import numpy as np
import pytest

import pfb_pspec_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EED0F5C
M = 64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def random_bytes(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def input_rows(P, K):
    """Input rows T per call.  One short of an output row (nothing to do); exactly P + K - 1 (one output row; for K < 16 fewer
    channelizer rows than one 16-row tile); where K < 16 the most whole output rows that fit in fewer than 16 channelizer rows; and
    2 runs of `least` output rows and a part of a third -- three wavefronts when a wave owns whole rows (the last one shorter and,
    unless K is a multiple of 16, ending inside a tile), more when it owns runs of four segments -- with K - 1 rows of a dropped row."""
    least = -(-64 // K)
    nrows = 2 * least + max(1, least * 37 // 64)
    T = [P + K - 2, P + K - 1, nrows * K + P - 1 + (K - 1)]
    if K < 16 and 15 // K > 1:
        T.insert(2, 15 // K * K + P - 1)
    return T


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("K", [1, 5, 16, 17, 40, 256])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_fused_bit_exact_in_every_mode(gpu, redio, oracle, P, K, fused):
    h = oracle.synth_f32(9, P, M * P)
    plan = redio.PolyphaseSpectrum(h, M, P, K, fused=fused)
    assert plan.is_fused
    for T in input_rows(P, K):
        x = oracle.synth_iq(SEED + K, T, M * T + 3)
        want = ref.spectrum(x, h, M, P, K, fused)
        assert want.shape == (max(T - P + 1, 0) // K, M) and plan.nrows(len(x)) == len(want)
        d = gpu.from_numpy(x).cuda()
        for mode in (plan.AUTO, plan.ROWS, plan.SEGMENTS):
            plan.set_split(mode)
            out = gpu.full((want.size + M,), 7.0, dtype=gpu.float32, device="cuda")
            got = plan(d, out=out)
            assert got.shape == want.shape
            assert np.array_equal(bits(got.cpu().numpy()), bits(want)), (T, mode)
            assert bool((out[want.size:] == 7.0).all()), (T, mode)  # nothing behind the rows, and nothing at all without a row


@pytest.mark.parametrize("K", [1, 17, 256])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_fused_against_the_composition_on_the_gpu(gpu, redio, oracle, P, K):
    """2^18 samples: Channelizer followed by PowerSpectrum(64, K).spectra gives the same bits; K = 1 is numpy's re * re + im * im
    of the channelizer's rows"""
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    x = redio.synth_iq(SEED, 0, 1 << 18)
    rows = redio.Channelizer(h, M, P)(x)
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    want = redio.PowerSpectrum(M, K).spectra(rows[: len(rows) // K * K])
    for mode in (plan.AUTO, plan.ROWS, plan.SEGMENTS):
        plan.set_split(mode)
        got = plan(x)
        assert got.shape == want.shape == (((1 << 18) // M - P + 1) // K, M)
        assert gpu.equal(got.view(gpu.int32), want.view(gpu.int32)), mode
    if K == 1:
        r = rows.cpu().numpy()
        assert np.array_equal(bits(got.cpu().numpy()), bits(r.real * r.real + r.imag * r.imag))


@pytest.mark.parametrize("off", [0, 2])
@pytest.mark.parametrize("K", [5, 40])
@pytest.mark.parametrize("P", [4, 8, 16])
def test_fused_from_bytes(gpu, redio, oracle, P, K, off):
    """u8 I/Q bytes at byte offsets 0 and 2 of an aligned allocation: the restatement's bits, and those of data_to_samples followed
    by the cf32 call, in every mode"""
    h = oracle.synth_f32(5, P, M * P)
    T = input_rows(P, K)[-1]
    raw = random_bytes(SEED + P + K, 2 * (M * T + 3) + off)
    big = gpu.from_numpy(raw).cuda()
    assert big.data_ptr() % 16 == 0
    rd = big[off:]
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    want = ref.spectrum_u8(raw[off:], h, M, P, K, True)
    via_cf32 = plan(redio.bitfount.data_to_samples(rd))
    assert np.array_equal(bits(via_cf32.cpu().numpy()), bits(want))
    for mode in (plan.AUTO, plan.ROWS, plan.SEGMENTS):
        plan.set_split(mode)
        got = plan.from_bytes(rd)
        assert got.shape == want.shape and gpu.equal(got.view(gpu.int32), via_cf32.view(gpu.int32)), mode


@pytest.mark.parametrize("rows", [1, 17, 33, 2048 + 5])
def test_byte_stream_ends_at_a_guard_region(gpu, redio, oracle, rows):
    """as test_channelizer_u8_stream_ends_at_a_guard_region: the byte stream is a view that ends exactly where 4 KiB of 0xFF bytes
    begin; rows past the end of the stream are never part of a result"""
    P, K = 16, 3
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    nbytes = 2 * M * (rows + P - 1)
    raw = random_bytes(rows, nbytes)
    big = gpu.full((nbytes + 4096,), 255, dtype=gpu.uint8, device="cuda")
    big[:nbytes] = gpu.from_numpy(raw).cuda()
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    want = ref.spectrum_u8(raw, h, M, P, K, True)
    for mode in (plan.ROWS, plan.SEGMENTS):
        plan.set_split(mode)
        got = plan.from_bytes(big[:nbytes]).cpu().numpy()
        assert got.shape == want.shape == (rows // K, M) and np.array_equal(bits(got), bits(want)), mode


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("Mg,P,K", [(128, 8, 17), (100, 5, 5), (128, 8, 1)])
def test_generic_bit_exact(gpu, redio, oracle, Mg, P, K, fused):
    """shapes of test_channelizer_any_channel_count -- 128 x 8 is one of the channelizer's one-kernel shapes, 100 x 5 runs its two
    passes -- through the plan's own channelizer, the accumulate pass and the fold, from cf32 and from bytes at offset 2"""
    h = oracle.synth_f32(9, 0, Mg * P)
    plan = redio.PolyphaseSpectrum(h, Mg, P, K, fused=fused)
    assert not plan.is_fused
    for T in (P + K - 2, P + K - 1, 3 * K + P - 1 + (K - 1)):
        x = oracle.synth_iq(SEED + Mg, T, Mg * T + 3)
        want = ref.spectrum(x, h, Mg, P, K, fused)
        got = plan(gpu.from_numpy(x).cuda())
        assert got.shape == want.shape == (max(T - P + 1, 0) // K, Mg)
        assert np.array_equal(bits(got.cpu().numpy()), bits(want)), T
        raw = random_bytes(SEED + T, 2 * (Mg * T + 3) + 2)
        want = ref.spectrum_u8(raw[2:], h, Mg, P, K, fused)
        got = plan.from_bytes(gpu.from_numpy(raw).cuda()[2:])
        assert got.shape == want.shape and np.array_equal(bits(got.cpu().numpy()), bits(want)), T


def test_generic_across_the_chunk_seam(gpu, redio, oracle):
    """64 x 5, K = 32: a pass through the row scratch takes 8192 segments (64 MiB of rows); 4100 rows of two segments are 8200, so
    the last eight go through a second pass -- about 2^23 samples.  Against the composition on the GPU, from cf32 and from bytes."""
    P, K, nrows = 5, 32, 4100
    h = oracle.synth_f32(9, 0, M * P)
    n = M * (nrows * K + P - 1) + 7
    x = redio.synth_iq(SEED, 0, n)
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    assert not plan.is_fused and plan.nrows(n) == nrows
    integ = redio.PowerSpectrum(M, K)
    want = integ.spectra(redio.Channelizer(h, M, P)(x)[: nrows * K])
    got = plan(x)
    assert got.shape == want.shape == (nrows, M) and gpu.equal(got.view(gpu.int32), want.view(gpu.int32))
    del x, want, got
    raw = gpu.from_numpy(random_bytes(SEED, 2 * n)).cuda()
    want = integ.spectra(redio.Channelizer(h, M, P).from_bytes(raw)[: nrows * K])
    got = plan.from_bytes(raw)
    assert gpu.equal(got.view(gpu.int32), want.view(gpu.int32))
