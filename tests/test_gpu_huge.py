"""Streams beyond 2^32 bytes, 2^31 and 2^32 elements (an MI355X holds 288 GB: one call may be handed that much).

Every kernel here was written with 64-bit unit indices and 32-bit offsets inside a unit; nothing but a run at these sizes shows that no
32-bit product crept in.  One cf32 stream of 2^32 + a ragged tail samples (34 GB) is generated on the device by the closed-form hash
 and pushed through each operator; the oracle recomputes, from nothing but its own input window, the outputs next to every
boundary that matters: the start, byte offset 2^32 (sample 2^29), element 2^31, element 2^32, the end.  Bit-exact, as everywhere.
The real-input and spectrum plans read narrower views of the same memory as f32 samples and as u8 I/Q bytes (second half of this file).
The three two-pass filterbank plans (synthesis bank, oversampled channelizer, oversampled synthesis bank) read it as samples or as rows
of channel values, on the wave route and down route 0 through hundreds of default passes (last part of this file).
The three workgroup kernels (the Channelizer's at 32 to 1024 channels, the polyphase spectrometer's and the oversampled channelizer's
with one_kernel=True) run on it as well: their index arithmetic is their own.
Skipped when the device has less than 120 GB free."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SEED = 0x5EED0009
N = (1 << 32) + 13 * 5120 + 1000  # cf32 samples


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def marks(total, unit=1):
    """unit indices next to the boundaries, for a stream of `total` units of `unit` samples each"""
    m = {0, total - 1}
    for p in (1 << 29, 1 << 31, 1 << 32):
        for q in (p // unit - 1, p // unit, p // unit + 1):
            if 0 <= q < total:
                m.add(q)
    return sorted(m)


@pytest.fixture(scope="module")
def big(gpu, redio):
    free, _ = gpu.cuda.mem_get_info()
    if free < 120 << 30:
        pytest.skip(f"needs 120 GB of free device memory, {free >> 30} GB free")
    x = redio.synth_iq(SEED, 0, N)
    yield x
    del x
    gpu.cuda.empty_cache()


def test_synth_past_2_32(gpu, redio, oracle, big):
    for p in marks(N):
        lo = max(0, p - 100)
        hi = min(N, p + 100)
        assert same_bits(big[lo:hi].cpu().numpy(), oracle.synth_iq(SEED, lo, hi - lo)), p


@pytest.mark.parametrize("k,d,fused", [(127, 5, True), (127, 5, False), (63, 1, False), (100, 3, False), (7, 13, False)])
def test_fir_past_2_32(gpu, redio, oracle, big, k, d, fused):
    """dsputils::convolve (dsputils.rs:30-32) with decimation: the chain kernel's FIR-only form, the tiled, the chunked and the direct kernel"""
    taps = oracle.lpf_corrected(k, 0.08)
    fir = redio.Fir(taps, d, complex_input=True, fused=fused)
    nout = fir.nout(N)
    assert nout == (N - k) // d + 1
    out = fir(big)
    assert out.numel() == nout
    for p in marks(N):
        o0 = max(0, min(p // d - 700, nout - 1400))
        cnt = min(1400, nout - o0)
        xw = oracle.synth_iq(SEED, o0 * d, (cnt - 1) * d + k)
        want = oracle.fir(xw, taps, d, fused=fused)
        assert same_bits(out[o0:o0 + cnt].cpu().numpy(), want), (k, d, p)
    del out


@pytest.mark.parametrize("nfft", [1024, 64, 4096, 16384, 65536, 1000])
def test_fft_past_2_32(gpu, redio, oracle, big, nfft):
    """kissfft::fft (kissfft.rs:18-31) on consecutive blocks of the stream"""
    nb = N // nfft
    plan = redio.Fft(nfft)
    out = plan(big[: nb * nfft])
    for b in marks(nb, nfft):
        lo = max(0, min(b - 1, nb - 3))
        cnt = min(3, nb - lo)
        want = oracle.fft(oracle.synth_iq(SEED, lo * nfft, cnt * nfft), nfft)
        assert same_bits(out[lo * nfft:(lo + cnt) * nfft].cpu().numpy().reshape(cnt, nfft), want.reshape(cnt, nfft)), (nfft, b)
    del out


def test_chain_past_2_32(gpu, redio, oracle, big):
    """BASELINE.json configs[1] sixteen times over: 838 873 blocks in one launch"""
    taps = oracle.lpf_corrected(127, 0.08)
    for fused in (True, False):
        chain = redio.Chain(taps, 5, 1024, fused=fused)
        nb = chain.nblocks(N)
        assert nb == ((N - 127) // 5 + 1) // 1024
        out = chain(big)
        for b in marks(nb, 5120):
            lo = max(0, min(b - 4, nb - 9))
            cnt = min(9, nb - lo)
            want = oracle.chain_fir_fft(oracle.synth_iq(SEED, lo * 5120, cnt * 5120 + 126), taps, 5, 1024, fused=fused)
            assert same_bits(out[lo:lo + cnt].cpu().numpy(), want), (fused, b)
        del out


def test_channelizer_past_2_32(gpu, redio, oracle, big):
    """BASELINE.json configs[3]: 64 channels, 16 taps per branch, 2^26 rows"""
    M, P = 64, 16
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    plan = redio.Channelizer(h, M, P)
    rows = plan.nrows(N)
    out = plan(big)
    assert tuple(out.shape) == (rows, M)
    for r in marks(rows, M):
        lo = max(0, min(r - 20, rows - 40))
        cnt = min(40, rows - lo)
        want = oracle.pfb_channelizer(oracle.synth_iq(SEED, lo * M, (cnt + P - 1) * M), h, M, P, fused=True)
        assert same_bits(out[lo:lo + cnt].cpu().numpy(), want[:cnt]), r
    del out
    # the per-destination layout of the exchange step: [group][row][M / groups]
    g = 8
    outg = plan(big, ngroups=g)
    for r in marks(rows, M):
        lo = max(0, min(r - 20, rows - 40))
        cnt = min(40, rows - lo)
        want = oracle.pfb_channelizer(oracle.synth_iq(SEED, lo * M, (cnt + P - 1) * M), h, M, P, fused=True)[:cnt]
        got = outg[:, lo:lo + cnt, :].cpu().numpy()
        assert same_bits(np.ascontiguousarray(got.transpose(1, 0, 2)).reshape(cnt, M), want), r
    del outg


@pytest.mark.parametrize("M,P,groups", [(32, 4, 1), (512, 16, 8), (1024, 8, 1)])
def test_channelizer_workgroup_kernel_past_2_32(gpu, redio, oracle, big, M, P, groups):
    """pfb_p2_kernel, the workgroup kernel of 32 to 1024 channels, on the whole stream: its index arithmetic is not the wave kernel's
    (rows per stream, streams per workgroup, row * M + n); one shape also in the grouped layout [group][row][M / groups]"""
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    plan = redio.Channelizer(h, M, P)
    rows = plan.nrows(N)
    assert rows == N // M - P + 1 and rows * M > 1 << 32 and N * 8 > 1 << 35
    for g in sorted({1, groups}):
        out = plan(big, ngroups=g)
        assert out.numel() == rows * M and tuple(out.shape) == ((rows, M) if g == 1 else (g, rows, M // g))
        for r in marks(rows, M):
            lo = max(0, min(r - 20, rows - 40))
            cnt = min(40, rows - lo)
            want = oracle.pfb_channelizer(oracle.synth_iq(SEED, lo * M, (cnt + P - 1) * M), h, M, P, fused=True)[:cnt]
            got = out[lo:lo + cnt].cpu().numpy() if g == 1 else np.ascontiguousarray(out[:, lo:lo + cnt, :].cpu().numpy().transpose(1, 0, 2)).reshape(cnt, M)
            assert same_bits(got, want), (g, r)
        del out


@pytest.mark.parametrize("nfft,k", [(65536, 8193), (4096, 127), (32768, 127)])
def test_overlap_save_past_2_32(gpu, redio, oracle, big, nfft, k):
    """BASELINE.json configs[4]: blocks of nfft points, hop nfft - k + 1, through the chunk loop tens of thousands of times"""
    h = oracle.lpf_corrected(k, 0.08)
    plan = redio.OverlapSave(h, nfft)
    hop = nfft - k + 1
    nout = plan.nout(N)
    out = plan(big)
    assert out.numel() == nout and nout % hop == 0
    nblk = nout // hop
    for b in marks(nblk, hop):
        lo = max(0, min(b - 1, nblk - 2))
        cnt = min(2, nblk - lo)
        want = oracle.overlap_save(oracle.synth_iq(SEED, lo * hop, (cnt - 1) * hop + nfft), h, nfft)
        assert same_bits(out[lo * hop:(lo + cnt) * hop].cpu().numpy(), want[: cnt * hop]), (nfft, b)
    del out


def test_ingest_past_2_32(gpu, redio, oracle, big):
    """rtlsdr::data_to_samples (rtlsdr.rs:159-162), norm, the 512-sample block sums and discretize (bitfount.rs:36-96) on 2^33 bytes / 2^32 samples"""
    raw = gpu.view_as_real(big).view(gpu.int32).reshape(-1)  # two words per sample
    d = ((raw >> 9) & 255).to(gpu.uint8)                      # one byte per word: 2 N bytes = N I/Q pairs
    del raw

    def host_bytes(first, n):  # the same bytes from the hash, samples [first, first + n)
        return ((oracle.synth_iq(SEED, first, n).view(np.int32).reshape(-1) >> 9) & 255).astype(np.uint8)

    x = redio.bitfount.data_to_samples(d)
    assert x.numel() == N
    for p in marks(N):
        lo, hi = max(0, p - 300), min(N, p + 300)
        assert same_bits(x[lo:hi].cpu().numpy(), oracle.data_to_samples(host_bytes(lo, hi - lo))), p
    del x
    mag = redio.bitfount.ingest_mag(d)
    for p in marks(N):
        lo, hi = max(0, p - 300), min(N, p + 300)
        assert same_bits(mag[lo:hi].cpu().numpy(), oracle.norm(oracle.data_to_samples(host_bytes(lo, hi - lo)))), p
    del d
    sums = redio.bitfount.block_sums(mag, 512)
    nb = N // 512
    assert sums.numel() == nb
    for b in marks(nb, 512):
        m = oracle.norm(oracle.data_to_samples(host_bytes(b * 512, 512)))
        assert bits(sums[b:b + 1].cpu().numpy())[0] == bits(np.array([oracle.block_sum(m)], np.float32))[0], b
    del sums
    mag[N - 5] = 3.0  # the maximum sits behind element 2^32
    sl = redio.bitfount.discretize(mag)
    assert sl.numel() == N
    for p in marks(N):
        lo, hi = max(0, p - 300), min(N, p + 300)
        m = oracle.norm(oracle.data_to_samples(host_bytes(lo, hi - lo)))
        if lo <= N - 5 < hi:
            m[N - 5 - lo] = 3.0
        assert np.array_equal(sl[lo:hi].cpu().numpy(), (m > np.float32(1.5)).astype(np.uint8)), p
    del sl, mag


def test_resampler_past_2_32(gpu, redio, oracle, big):
    """BASELINE.json configs[2] with 2^32 frames in one message: 256 channels x 2^24 frames, ratio 0.02"""
    nch, n, ratio = 256, 1 << 24, 0.02
    d = gpu.view_as_real(big).reshape(-1)[: nch * n].reshape(nch, n)  # channel c = f32 words [c n, (c + 1) n) of the stream
    src = redio.Src(nch, 1)
    out, used = src.process(d, ratio)
    assert used == n
    for c in (0, 127, 128, 255):  # channel 128 starts at element 2^31
        w = oracle.synth_iq(SEED, c * n // 2, n // 2).view(np.float32).reshape(-1)
        err, want, wused = oracle.Resampler(1).process(w, ratio, int(ratio * n + 1.0))
        assert err == 0 and wused == n
        assert same_bits(out[c].cpu().numpy(), want), c


# ---- the real-input and spectrum plans --------------------------------------------------------------------------------------------------
# The same stream seen three ways: cf32 samples, and -- narrower views of its first bytes -- NV f32 samples and NV u8 I/Q byte pairs,
# so that element 2^32 of either view and byte offset 2^33 of the u8 one lie inside.  Every check recomputes the rows next to a mark
# from its own window of the hash, through the restatements of tests/ (pspec_ref, pspec_real_ref, fftr_ref, ovsave_real_ref).
NV = N


def f32_view(gpu, big):
    return gpu.view_as_real(big).reshape(-1)[:NV]


def u8_view(gpu, big):
    return gpu.view_as_real(big).reshape(-1).view(gpu.uint8)[: 2 * NV]


def host_f32(oracle, lo, cnt):
    """f32 words [lo, lo + cnt) of the stream"""
    c0 = lo // 2
    return oracle.synth_iq(SEED, c0, (lo + cnt + 1) // 2 - c0).view(np.float32)[lo - 2 * c0: lo - 2 * c0 + cnt]


def host_u8(oracle, lo, cnt):
    """the bytes of u8 I/Q samples [lo, lo + cnt) of the stream"""
    b0, b1 = 2 * lo, 2 * (lo + cnt)
    c0 = b0 // 8
    return oracle.synth_iq(SEED, c0, (b1 + 7) // 8 - c0).view(np.uint8)[b0 - 8 * c0: b1 - 8 * c0]


def check_rows(out, rows, W, H, want_of, more=()):
    """rows of `out` next to every mark (and the rows `more` names) against want_of(first sample, sample count)"""
    for b in sorted(set(marks(rows, H)) | {q for q in more if 0 <= q < rows}):
        lo = max(0, min(b - 1, rows - 3))
        cnt = min(3, rows - lo)
        assert same_bits(out[lo:lo + cnt].cpu().numpy(), want_of(lo * H, (cnt - 1) * H + W)), b


@pytest.mark.parametrize("nfft,k,step,windowed,mode", [(1024, 16, 1024, False, 1), (1024, 16, 1024, False, 2), (1024, 17, 1024, False, 2), (4096, 4, 4096, False, 0), (1024, 4, 512, True, 0)])
def test_pspec_past_2_32(gpu, redio, oracle, big, nfft, k, step, windowed, mode):
    """redio_pspec_enqueue: the fused kernel over 262 148 rows (1 GiB out) in both launch modes (at K = 16 a row is one segment, so
    both launch a wave per row; K = 17 in mode 2 is the wave per segment with its 2 GiB of partials and the fold pass), the generic
    path's chunk loop 2048 times over at 4096 points, and the fused kernel on overlapping windowed rows (2^21 of them)"""
    import pspec_ref
    w = oracle.lpf_corrected(nfft, 0.1) if windowed else None
    W, H = pspec_ref.shape(nfft, k, step)
    plan = redio.PowerSpectrum(nfft, k, step, w)
    plan.set_split(mode)
    rows = plan.nrows(N)
    assert rows == (N - W) // H + 1 and plan.is_fused == (nfft == 1024)
    out = plan(big)
    assert tuple(out.shape) == (rows, nfft)
    check_rows(out, rows, W, H, lambda lo, cnt: pspec_ref.power_spectrum(oracle.synth_iq(SEED, lo, cnt), nfft, k, step, w))
    del out


@pytest.mark.parametrize("nfft,k", [(1024, 16), (2048, 4), (1000, 4)])
def test_pspec_u8_past_2_32(gpu, redio, oracle, big, nfft, k):
    """redio_pspec_enqueue_u8 on 2^33 bytes and more: the fused kernel, the transform that converts at its own load (2048) and the
    converting row gather (1000), whose 32-bit indices inside a chunk hold only because a chunk is small: there the rows either side of
    the chunk seams next to every mark are compared as well"""
    import pspec_ref
    raw = u8_view(gpu, big)
    assert raw.numel() == 2 * NV > 1 << 33
    W, H = pspec_ref.shape(nfft, k, nfft)
    plan = redio.PowerSpectrum(nfft, k)
    rows = plan.nrows(NV)
    assert rows == (NV - W) // H + 1
    out = plan.u8(raw)
    assert tuple(out.shape) == (rows, nfft)
    chunk = max(1, (64 << 20) // (nfft * 8 * pspec_ref.SEG))   # rows per pass of the generic path (one segment per row at this K)
    seams = [q for b in marks(rows, H) for q in (b // chunk * chunk, (b // chunk + 1) * chunk)] if nfft != 1024 else []
    check_rows(out, rows, W, H, lambda lo, cnt: pspec_ref.power_spectrum(oracle.data_to_samples(host_u8(oracle, lo, cnt)), nfft, k), seams)
    del out


@pytest.mark.parametrize("M,P,K,mode,u8", [(64, 16, 16, 1, False), (64, 16, 17, 2, False), (64, 4, 16, 0, True), (128, 8, 16, 0, False), (100, 5, 4, 0, False)])
def test_pfb_pspec_past_2_32(gpu, redio, oracle, big, M, P, K, mode, u8):
    """redio_pfb_pspec_enqueue on 2^32 samples and more: the fused 64-channel kernel with a wave per run of whole rows, with a wave per
    run of segments (K = 17: about 2 GiB of partials, and the fold pass) and from more than 2^33 bytes of u8 I/Q; the generic path through
    its chunk loop on a one-kernel shape of the channelizer (128 x 8) and a two-pass one (100 x 5), where the rows either side of the
    chunk seams next to every mark are compared as well"""
    import pfb_pspec_ref
    import pspec_ref
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    W, H = pfb_pspec_ref.shape(M, P, K)
    plan = redio.PolyphaseSpectrum(h, M, P, K)
    plan.set_split(mode)
    rows = plan.nrows(NV)
    assert rows == (NV - W) // H + 1 and plan.is_fused == (M == 64)
    if u8:
        raw = u8_view(gpu, big)
        assert raw.numel() == 2 * NV > 1 << 33
        out = plan.from_bytes(raw)
        want_of = lambda lo, cnt: pfb_pspec_ref.spectrum_u8(host_u8(oracle, lo, cnt), h, M, P, K, True)
    else:
        out = plan(big)
        want_of = lambda lo, cnt: pfb_pspec_ref.spectrum(oracle.synth_iq(SEED, lo, cnt), h, M, P, K, True)
    assert tuple(out.shape) == (rows, M)
    assert K <= pspec_ref.SEG or plan.is_fused                 # below: a generic row is one segment
    chunk = max(1, (64 << 20) // (M * 8 * pspec_ref.SEG))      # rows per pass of the generic path
    seams = [q for b in marks(rows, H) for q in (b // chunk * chunk, (b // chunk + 1) * chunk)] if not plan.is_fused else []
    check_rows(out, rows, W, H, want_of, seams)
    del out


@pytest.mark.parametrize("M,P,K,mode,u8", [(128, 8, 16, 1, False), (1024, 4, 17, 2, False), (32, 16, 4, 0, True)])
def test_pfb_pspec_workgroup_kernel_past_2_32(gpu, redio, oracle, big, M, P, K, mode, u8):
    """redio_pfb_pspec_enqueue with one_kernel=True (route 2) on 2^32 samples and more: a thread group per run of whole rows, per run of
    segments (K = 17: about 2 GiB of partials, and the fold pass), and from more than 2^33 bytes of u8 I/Q.  The rows either side of the
    row streams' boundaries next to every mark are compared as well (the launch geometry restated in tests/fuzz_spectra.py)."""
    import fuzz_spectra
    import pfb_pspec_ref
    import pspec_ref
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    W, H = pfb_pspec_ref.shape(M, P, K)
    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
    plan.set_split(mode)
    rows = plan.nrows(NV)
    assert rows == (NV - W) // H + 1 and plan.route == 2 and not plan.is_fused
    assert rows * K * M > 1 << 32   # channelizer rows times channels: the elements the kernel's row indices address
    if u8:
        raw = u8_view(gpu, big)
        assert raw.numel() == 2 * NV > 1 << 33
        out = plan.from_bytes(raw)
        want_of = lambda lo, cnt: pfb_pspec_ref.spectrum_u8(host_u8(oracle, lo, cnt), h, M, P, K, True)
    else:
        assert NV * 8 > 1 << 35
        out = plan(big)
        want_of = lambda lo, cnt: pfb_pspec_ref.spectrum(oracle.synth_iq(SEED, lo, cnt), h, M, P, K, True)
    assert tuple(out.shape) == (rows, M)
    g = fuzz_spectra.pfb_block_geometry(M, K, rows, mode, gpu.cuda.get_device_properties(0).multi_processor_count)
    S = -(-K // pspec_ref.SEG) if g["split"] else 1
    assert g["split"] == (K > pspec_ref.SEG) and g["units"] == rows * S and g["groups"] > 100
    if g["split"]:
        assert g["units"] * M * 4 > 15 << 27   # the partials: about 2 GiB
    seams = [q for b in marks(rows, H) for q in ((b * S // g["ups"]) * g["ups"] // S, -(-(b * S // g["ups"] + 1) * g["ups"] // S))]
    check_rows(out, rows, W, H, want_of, seams)
    del out


@pytest.mark.parametrize("nfft,k,mode", [(2048, 16, 1), (2048, 16, 2), (2048, 17, 2), (4096, 4, 0)])
def test_pspec_real_past_2_32(gpu, redio, oracle, big, nfft, k, mode):
    """redio_pspec_real_enqueue on 2^32 f32 samples and more: the fused kernel in both launch modes (one segment per row at K = 16;
    K = 17 in mode 2 runs a wave per segment and the fold pass) and the generic path, whose transform reads the caller's buffer row by
    row through the chunk loop"""
    import pspec_real_ref
    x = f32_view(gpu, big)
    W, H = pspec_real_ref.shape(nfft, k, nfft)
    plan = redio.PowerSpectrumReal(nfft, k)
    plan.set_split(mode)
    rows = plan.nrows(NV)
    assert rows == (NV - W) // H + 1 and plan.is_fused == (nfft == 2048)
    out = plan(x)
    assert tuple(out.shape) == (rows, nfft // 2 + 1)
    check_rows(out, rows, W, H, lambda lo, cnt: pspec_real_ref.power_spectrum(host_f32(oracle, lo, cnt), nfft, k))
    del out


@pytest.mark.parametrize("nfft", [2048, 1000])
def test_fftr_past_2_32(gpu, redio, oracle, big, nfft):
    """kiss_fftr over consecutive frames of 2^32 f32 samples (fused at 2048, the complex plan and the split pass at 1000): more than
    2^31 bins come out, and kiss_fftri then takes five rows of them that lie across element 2^31 of that buffer"""
    import fftr_ref
    x = f32_view(gpu, big)
    nb, nbins = NV // nfft, nfft // 2 + 1
    assert nb * nbins > 1 << 31
    plan = redio.Fftr(nfft)
    assert plan.is_fused == (nfft == 2048)
    out = plan(x[: nb * nfft]).view(nb, nbins)
    check_rows(out, nb, nfft, nfft, lambda lo, cnt: fftr_ref.fftr_rows(host_f32(oracle, lo, cnt), nfft))
    r0 = (1 << 31) // nbins - 2
    assert r0 * nbins < 1 << 31 < (r0 + 5) * nbins
    back = redio.Fftr(nfft, inverse=True)(out[r0:r0 + 5].reshape(-1)).view(5, nfft)
    want = fftr_ref.fftri_rows(fftr_ref.fftr_rows(host_f32(oracle, r0 * nfft, 5 * nfft), nfft), nfft)
    assert same_bits(back.cpu().numpy(), want)
    del out, back


@pytest.mark.parametrize("nfft,ntaps", [(2048, 127), (4096, 1025)])
def test_ovsave_real_past_2_32(gpu, redio, oracle, big, nfft, ntaps):
    """redio_ovsave_real_enqueue on 2^32 f32 samples and more: the fused kernel, and the generic path through its chunk loop"""
    import ovsave_real_ref
    x = f32_view(gpu, big)
    h = oracle.lpf_corrected(ntaps, 0.08)
    plan = redio.OverlapSaveReal(h, nfft)
    hop = nfft - ntaps + 1
    nout = plan.nout(NV)
    assert nout == ((NV - nfft) // hop + 1) * hop > 1 << 32 and plan.is_fused == (nfft == 2048)
    out = plan(x)
    assert out.numel() == nout
    for p in marks(nout):
        o0 = max(0, min(p - 700, nout - 1400))
        b0, b1 = o0 // hop, (o0 + 1399) // hop
        want = ovsave_real_ref.overlap_save_real(host_f32(oracle, b0 * hop, (b1 - b0) * hop + nfft), h, nfft)
        assert same_bits(out[o0:o0 + 1400].cpu().numpy(), want[o0 - b0 * hop: o0 - b0 * hop + 1400]), (nfft, p)
    del out


# ---- the polyphase banks --------------------------------------------------------------------------------------------------------------------
# The synthesis bank, the oversampled channelizer and the oversampled synthesis bank (one driver, pfb_bank.hip) on the stream, read as
# samples or as rows of channel values.  A unit is an output row, a row, or a hop: unit u reads `window` input elements from u * hop_in
# on and gives unit_out output elements.  Every check recomputes a few units next to a mark from their own window of the hash with
# first_row + the window's first unit, so that the window's reference is the call's.  The wave-route shapes run twice, the second time
# down route 0 with the chunk left alone: hundreds of default passes, input and output offsets above 2^32 elements, and there the units
# either side of the pass seams next to every mark are compared as well.
BANK_FIRST = 5   # first_row of every call: odd, so that the hop-32 plans turn their rows by 32 places from the start


def bank_geometry(kind, M, P, H):
    """(window, hop_in, unit_out, min_rows): pfb_bank_cut.h's table"""
    L = -(-M * P // H)
    return {"synth": (M * P, M, M, P), "os": (M * P, H, M, 1), "os_synth": (M * L, M, H, L)}[kind]


def bank_want(oracle, kind, h, M, P, H, lo, cnt):
    import pfb_os_ref
    import pfb_os_synth_ref
    import pfb_synth_ref
    window, hop_in, _, _ = bank_geometry(kind, M, P, H)
    x = oracle.synth_iq(SEED, lo * hop_in, (cnt - 1) * hop_in + window)
    if kind == "synth":
        return pfb_synth_ref.synth(x, h, M, P, True)
    if kind == "os":
        return pfb_os_ref.channelize(x, h, M, P, H, BANK_FIRST + lo, True).reshape(-1)
    return pfb_os_synth_ref.synth(x, h, M, P, H, BANK_FIRST + lo, True)


def check_bank(oracle, out, kind, h, M, P, H, units, at):
    _, _, unit_out, _ = bank_geometry(kind, M, P, H)
    for b in sorted({q for q in at if 0 <= q < units}):
        lo = max(0, min(b - 2, units - 5))
        cnt = min(5, units - lo)
        want = bank_want(oracle, kind, h, M, P, H, lo, cnt)
        assert same_bits(out[lo * unit_out:(lo + cnt) * unit_out].cpu().numpy(), want), (kind, M, P, H, b)


def run_bank_past_2_32(gpu, redio, oracle, big, kind, M, P, H, n_in, routes, one_kernel=False):
    """the call on the first n_in elements of the stream on every route of `routes`; returns (units, output elements).  one_kernel: the
    oversampled channelizer's plan with its workgroup kernel (route 2), where the units either side of the row streams' boundaries
    next to every mark are compared as well"""
    window, hop_in, unit_out, min_rows = bank_geometry(kind, M, P, H)
    h = oracle.lpf_corrected(M * P, 0.45 / M)
    plan = {"synth": lambda: redio.Synthesizer(h, M, P), "os": lambda: redio.OversampledChannelizer(h, M, P, H, one_kernel=one_kernel),
            "os_synth": lambda: redio.OversampledSynthesizer(h, M, P, H)}[kind]()
    units = (n_in - window) // hop_in + 1
    assert (plan.nrows(n_in) if kind == "os" else plan.nout(n_in) // unit_out) == units
    x = big[:n_in]
    at = set(marks(units, unit_out)) | set(marks(units, hop_in))   # next to the boundaries of the output and of the input
    for route in routes:
        plan.set_unfused(route == 0)
        assert plan.route == route
        seams = set()
        if route == 0:
            per = (64 << 20) // (M * 8) - min_rows + 1                # units per default pass (pfb_bank_cut.h)
            assert units > 100 * per or M != 64
            seams = {q for b in at for q in (b // per * per, (b // per + 1) * per)}
        if route == 2:
            import pfb_os_p2_ref as p2
            rps = p2.rows_per_stream(units, gpu.cuda.get_device_properties(0).multi_processor_count, M)   # rows of one stream of the launch
            assert units > 100 * rps
            seams = {q for b in at for q in (b // rps * rps, (b // rps + 1) * rps)}
        out = (plan(x) if kind == "synth" else plan(x, first_row=BANK_FIRST)).reshape(-1)
        assert out.numel() == units * unit_out
        check_bank(oracle, out, kind, h, M, P, H, units, at | seams)
        del out
    return units, units * unit_out


def test_pfb_synth_past_2_32(gpu, redio, oracle, big):
    """redio_pfb_synth_enqueue on the whole stream as 2^26 rows of 64 channel values: more than 2^32 samples out"""
    units, nout = run_bank_past_2_32(gpu, redio, oracle, big, "synth", 64, 16, 64, N, (1, 0))
    assert nout > 1 << 32


def test_pfb_os_past_2_32(gpu, redio, oracle, big):
    """redio_pfb_os_enqueue at hop 32 on the first 2^31 + 2^20 samples: more than 2^26 rows, so more than 2^32 elements out"""
    units, nout = run_bank_past_2_32(gpu, redio, oracle, big, "os", 64, 16, 32, (1 << 31) + (1 << 20), (1, 0))
    assert units > 1 << 26 and nout > 1 << 32


@pytest.mark.parametrize("M,P,H", [(32, 16, 16), (512, 8, 256), (1024, 4, 512)])
def test_pfb_os_workgroup_kernel_past_2_32(gpu, redio, oracle, big, M, P, H):
    """redio_pfb_os_enqueue with one_kernel=True (route 2) at hop M / 2 on the first 2^31 + 2^20 samples: more than 2^32 elements out,
    through half-row indices, rows per stream and row * M + n of the workgroup kernel"""
    n_in = (1 << 31) + (1 << 20)
    units, nout = run_bank_past_2_32(gpu, redio, oracle, big, "os", M, P, H, n_in, (2,), one_kernel=True)
    assert units == (n_in - M * P) // H + 1 and nout == units * M > 1 << 32 and n_in * 8 > 1 << 34


def test_pfb_os_synth_past_2_32(gpu, redio, oracle, big):
    """redio_pfb_os_synth_enqueue at hop 32 on the whole stream as rows: more than 2^32 elements in, more than 2^31 elements (and byte
    2^32) out"""
    units, nout = run_bank_past_2_32(gpu, redio, oracle, big, "os_synth", 64, 16, 32, N, (1, 0))
    assert units * 64 > 1 << 32 and nout > 1 << 31


def test_pfb_os_two_pass_shape_past_2_32(gpu, redio, oracle, big):
    """a shape with no wave kernel, (100, 3, 60): 2^32 / 100 rows and a thousand more, so the output passes 2^32 elements; 512 default
    passes of 83886 rows, where 64 MiB is no whole number of rows"""
    rows = (1 << 32) // 100 + 1000
    units, nout = run_bank_past_2_32(gpu, redio, oracle, big, "os", 100, 3, 60, 300 + (rows - 1) * 60 + 7, (0,))
    assert units == rows and nout > 1 << 32


def test_pfb_os_synth_two_pass_shape_past_2_32(gpu, redio, oracle, big):
    """(100, 3, 60), L = 5, on the whole stream as rows of 100: more than 2^32 elements in.  A hop gives 60 samples for 100 values, so
    the stream's 2^32 elements give 0.6 * 2^32 out: past element 2^31 and byte 2^32, short of element 2^32"""
    units, nout = run_bank_past_2_32(gpu, redio, oracle, big, "os_synth", 100, 3, 60, N, (0,))
    assert units * 100 > 1 << 32 and nout > 1 << 31
