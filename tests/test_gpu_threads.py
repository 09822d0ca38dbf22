"""Distinct handles from distinct threads (the reference runs one OS thread per block, src/ratpak.rs:60-185): the
library keeps no hidden global state, so concurrent plans must not disturb each other.  ctypes releases the GIL
during the calls, so these threads really overlap inside libredio."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_concurrent_plans_on_their_own_streams(gpu, redio, oracle):
    taps = oracle.lpf_corrected(127, 0.08)
    errors = []

    def worker(kind, seed):
        try:
            s = gpu.cuda.Stream()
            with gpu.cuda.stream(s):
                for it in range(12):
                    if kind == "chain":
                        x = oracle.synth_iq(seed + it, 0, 6 * 5120 + 126)
                        got = redio.Chain(taps, 5, 1024, fused=False)(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = oracle.chain_fir_fft(x, taps, 5, 1024, fused=False)
                    elif kind == "fft":
                        n = [64, 1000, 2048, 4096][it % 4]
                        x = oracle.synth_iq(seed + it, 0, n * 9)
                        got = redio.Fft(n)(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = oracle.fft(x, n)
                    elif kind == "fir":
                        k, d = [(64, 1), (127, 5), (33, 2), (255, 10)][it % 4]
                        h = oracle.synth_f32(seed, 0, k)
                        x = oracle.synth_iq(seed + it, 0, 20000)
                        got = redio.Fir(h, d)(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = oracle.fir(x, h, d, False)
                    elif kind == "conv":   # the host-buffer drop-in with its per-thread cache
                        u = oracle.synth_f32(seed + it, 0, 5000 + it)
                        got = redio.dsputils.convolve(u, taps)
                        want = oracle.convolve(u, taps)
                    else:                  # resampler state per thread
                        x = oracle.synth_f32(seed + it, 0, 30000)
                        got = redio.samplerate.State(1, 1).block(x, 0.02)
                        want = oracle.Resampler(1).block(x, 0.02)
                    if not (got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))):
                        errors.append((kind, it))
        except Exception as e:  # noqa: BLE001
            errors.append((kind, repr(e)))

    kinds = ["chain", "fft", "fir", "conv", "src", "chain", "fft", "conv"]
    threads = [threading.Thread(target=worker, args=(k, 1000 * (i + 1))) for i, k in enumerate(kinds)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not errors, errors


def test_concurrent_real_input_and_spectrum_plans(gpu, redio, oracle):
    """the plan families with plan-owned scratch that grows on first use (redio_pspec_*, its u8 entry, redio_pspec_real_*, the generic
    redio_fftr_* and redio_ovsave_real_*): eight threads, each with plans of its own on a stream of its own, messages whose length
    changes from call to call so that scratch regrows while the other threads are inside the library; every result bit for bit the
    restatement's"""
    import fftr_ref
    import ovsave_real_ref
    import pspec_real_ref
    import pspec_ref
    errors = []
    rows_of = [1, 3, 2, 5, 1, 4, 6, 2, 7, 3, 1, 8]   # per iteration: up and down, the largest last

    def worker(kind, seed):
        try:
            s = gpu.cuda.Stream()
            with gpu.cuda.stream(s):
                if kind == "pspec_fused":
                    N, K, step = 1024, 17, 512
                    w = oracle.lpf_corrected(N, 0.1)
                    plan = redio.PowerSpectrum(N, K, step, w)
                elif kind == "pspec_generic":   # K = 17: segment partials and row scratch
                    N, K, step = 96, 17, 48
                    w = oracle.lpf_corrected(N, 0.1)
                    plan = redio.PowerSpectrum(N, K, step, w)
                elif kind == "pspec_u8":
                    N, K, step, w = 64, 33, 64, None
                    plan = redio.PowerSpectrum(N, K, step)
                elif kind == "pspec_real4":     # un-windowed at step = N from a 4-byte base: the row gather instead of the caller's buffer
                    N, K, step, w = 1000, 17, 1000, None
                    plan = redio.PowerSpectrumReal(N, K, step)
                elif kind == "fftr":
                    N = 1000
                    plan = redio.Fftr(N)
                else:
                    N, taps = 1000, oracle.synth_f32(seed, 0, 101)
                    plan = redio.OverlapSaveReal(taps, N)
                for it, rows in enumerate(rows_of):
                    if kind == "pspec_fused":
                        rows = 1 + rows % 3
                    if kind.startswith("pspec"):
                        W, H = pspec_ref.shape(N, K, step)
                        n = W + (rows - 1) * H + 7 * it
                    if kind in ("pspec_fused", "pspec_generic"):
                        x = oracle.synth_iq(seed + it, 0, n)
                        got = plan(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = pspec_ref.power_spectrum(x, N, K, step, w)
                    elif kind == "pspec_u8":
                        raw = np.random.default_rng(seed + it).integers(0, 256, 2 * n, dtype=np.uint8)
                        buf = gpu.zeros(raw.size + 16, dtype=gpu.uint8, device="cuda")
                        buf[2: 2 + raw.size].copy_(gpu.from_numpy(raw))
                        got = plan.u8(buf[2: 2 + raw.size]).cpu().numpy()
                        want = pspec_ref.power_spectrum(oracle.data_to_samples(raw), N, K, step)
                    elif kind == "pspec_real4":
                        x = oracle.synth_f32(seed + it, 0, n)
                        buf = gpu.zeros(n + 4, dtype=gpu.float32, device="cuda")
                        buf[1: 1 + n].copy_(gpu.from_numpy(x))
                        assert buf[1:].data_ptr() % 8 == 4
                        got = plan(buf[1: 1 + n]).cpu().numpy()
                        want = pspec_real_ref.power_spectrum(x, N, K, step)
                    elif kind == "fftr":
                        x = oracle.synth_f32(seed + it, 0, 2 * rows * N)
                        got = plan(gpu.from_numpy(x).cuda()).cpu().numpy().reshape(-1, N // 2 + 1)
                        want = fftr_ref.fftr_rows(x, N)
                    else:
                        x = oracle.synth_f32(seed + it, 0, N + (rows - 1) * plan.hop + 13 * it)
                        got = plan(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = ovsave_real_ref.overlap_save_real(x, taps, N)
                    if not (got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))):
                        errors.append((kind, it))
        except Exception as e:  # noqa: BLE001
            errors.append((kind, repr(e)))

    kinds = ["pspec_fused", "pspec_generic", "pspec_u8", "pspec_real4", "fftr", "ovsave_real", "pspec_generic", "pspec_u8"]
    threads = [threading.Thread(target=worker, args=(k, 1000 * (i + 1))) for i, k in enumerate(kinds)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    assert not errors, errors


def test_concurrent_polyphase_spectrum_plans(gpu, redio, oracle):
    """redio_pfb_pspec_*: the segment partials of the fused kernel, the generic path's row scratch with the inner channelizer's own
    scratch behind it, the conversion scratch of its u8 entry, and a stream's carried history -- eight threads, each with a plan of its
    own on a stream of its own, row counts that rise and fall so that scratch regrows while the other threads are inside the library;
    every result bit for bit the restatement's"""
    import pfb_pspec_ref as ref
    errors = []
    rows_of = [1, 3, 2, 5, 1, 4, 6, 2, 7, 3, 1, 8]   # per iteration: up and down, the largest last

    def same(got, want):
        return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))

    def worker(kind, seed):
        try:
            s = gpu.cuda.Stream()
            with gpu.cuda.stream(s):
                M, P, K = {"fused": (64, 16, 17), "generic": (100, 5, 17), "generic_u8": (100, 5, 17), "stream": (64, 4, 3)}[kind]
                W, H = ref.shape(M, P, K)
                h = oracle.synth_f32(seed, 0, M * P)
                plan = redio.PolyphaseSpectrum(h, M, P, K)
                assert plan.is_fused == (M == 64)
                if kind == "stream":   # one stream in twelve pieces against the one-shot rows of the whole
                    lens = [(W - H if it == 0 else 0) + rows * H + 7 * it for it, rows in enumerate(rows_of)]
                    x = oracle.synth_iq(seed, 0, sum(lens))
                    whole = ref.spectrum(x, h, M, P, K, True)
                    d = gpu.from_numpy(x).cuda()
                    st = redio.Stream(plan)
                    pos = made = 0
                    for it, n in enumerate(lens):
                        got = st(d[pos: pos + n]).cpu().numpy().reshape(-1, M)
                        pos += n
                        now = ref.nrows(pos, M, P, K)
                        if not (same(got, whole[made:now]) and st.pending == pos - now * H):
                            errors.append((kind, it))
                        made = now
                    assert made == len(whole) >= sum(rows_of)
                    return
                for it, rows in enumerate(rows_of):
                    if kind == "fused":
                        rows *= 3   # runs of four segments: several wavefronts
                    n = W + (rows - 1) * H + 7 * it
                    if kind == "generic_u8":
                        raw = np.random.default_rng(seed + it).integers(0, 256, 2 * n, dtype=np.uint8)
                        buf = gpu.zeros(raw.size + 16, dtype=gpu.uint8, device="cuda")
                        buf[2: 2 + raw.size].copy_(gpu.from_numpy(raw))
                        got = plan.from_bytes(buf[2: 2 + raw.size]).cpu().numpy()
                        want = ref.spectrum_u8(raw, h, M, P, K, True)
                    else:
                        x = oracle.synth_iq(seed + it, 0, n)
                        got = plan(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = ref.spectrum(x, h, M, P, K, True)
                    if not (len(want) == rows and same(got, want)):
                        errors.append((kind, it))
        except Exception as e:  # noqa: BLE001
            errors.append((kind, repr(e)))

    kinds = ["fused", "generic", "generic_u8", "stream", "fused", "generic", "generic_u8", "stream"]
    threads = [threading.Thread(target=worker, args=(k, 1000 * (i + 1))) for i, k in enumerate(kinds)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"
    assert not errors, errors


def test_concurrent_polyphase_bank_plans(gpu, redio, oracle):
    """redio_pfb_synth_*, redio_pfb_os_*, redio_pfb_os_synth_* (one driver, pfb_bank.hip): each family on the wave route, on a two-pass
    shape with a small chunk (plan-owned scratch and the transform behind it) and as a stream fed in twelve pieces -- nine threads, each
    with a plan of its own on a stream of its own, unit counts that rise and fall so that scratch regrows while the other threads are
    inside the library; two of the threads create and drop a fresh plan every iteration, so that a destroy runs while the others
    enqueue; every result bit for bit the restatement's"""
    import pfb_os_ref
    import pfb_os_synth_ref
    import pfb_synth_ref
    errors = []
    rows_of = [1, 3, 2, 5, 1, 4, 6, 2, 7, 3, 1, 8]   # per iteration: up and down, the largest last
    FIRST = 3

    def same(got, want):
        return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))

    def geometry(fam, M, P, H):
        """(window, hop, unit_out, min_rows) in elements: pfb_bank_cut.h's table"""
        L = -(-M * P // H)
        return {"synth": (M * P, M, M, P), "os": (M * P, H, M, 1), "os_synth": (M * L, M, H, L)}[fam]

    def make(fam, h, M, P, H):
        if fam == "synth":
            return redio.Synthesizer(h, M, P)
        return (redio.OversampledChannelizer if fam == "os" else redio.OversampledSynthesizer)(h, M, P, H)

    def want_of(fam, x, h, M, P, H, F):
        if fam == "synth":
            return pfb_synth_ref.synth(x, h, M, P, True)
        if fam == "os":
            return pfb_os_ref.channelize(x, h, M, P, H, F, True).reshape(-1)
        return pfb_os_synth_ref.synth(x, h, M, P, H, F, True)

    def worker(how, fam, fresh, seed):
        try:
            s = gpu.cuda.Stream()
            with gpu.cuda.stream(s):
                M, P, H = (64, 4, 32) if how != "two_pass" else (100, 3, 60)
                H = M if fam == "synth" else H
                window, hop, unit_out, min_rows = geometry(fam, M, P, H)
                h = oracle.synth_f32(seed, 0, M * P)
                plan = make(fam, h, M, P, H)
                assert plan.route == (0 if how == "two_pass" else 1)
                if how == "stream":   # one stream in twelve pieces against the one-shot output of the whole, first_row = 0
                    lens = [(window - hop if it == 0 else 0) + rows * hop + 7 * it for it, rows in enumerate(rows_of)]
                    x = oracle.synth_iq(seed, 0, sum(lens))
                    whole = want_of(fam, x, h, M, P, H, 0)
                    d = gpu.from_numpy(x).cuda()
                    st = {"synth": redio.SynthesizerStream, "os": redio.OversampledChannelizerStream, "os_synth": redio.OversampledSynthesizerStream}[fam](plan)
                    pos = made = 0
                    for it, n in enumerate(lens):
                        got = st(d[pos: pos + n]).cpu().numpy()
                        pos += n
                        now = (pos - window) // hop + 1 if pos >= window else 0
                        if not (same(got, whole[made * unit_out: now * unit_out]) and st.pending == pos - now * hop):
                            errors.append((how, fam, it))
                        made = now
                    assert made * unit_out == len(whole) and made >= sum(rows_of)
                    return
                for it, rows in enumerate(rows_of):
                    if fresh and it:
                        plan = make(fam, h, M, P, H)   # the one before is dropped here: its destroy runs beside the other threads' calls
                    units = rows * 20 + it if how == "wave" else rows * 3   # wave: up to three wavefronts, odd and even counts
                    if how == "two_pass":
                        plan.set_chunk_rows(min_rows + 2)                   # passes of three units
                    x = oracle.synth_iq(seed + it, 0, (units - 1) * hop + window + 7 * it % hop)
                    d = gpu.from_numpy(x).cuda()
                    got = (plan(d) if fam == "synth" else plan(d, first_row=FIRST + it)).reshape(-1).cpu().numpy()
                    want = want_of(fam, x, h, M, P, H, FIRST + it)
                    if not (len(want) == units * unit_out and same(got, want)):
                        errors.append((how, fam, it))
        except Exception as e:  # noqa: BLE001
            errors.append((how, fam, repr(e)))

    jobs = [(how, fam, (how, fam) in (("wave", "synth"), ("two_pass", "os"))) for how in ("wave", "two_pass", "stream") for fam in ("synth", "os", "os_synth")]
    threads = [threading.Thread(target=worker, args=(how, fam, fresh, 1000 * (i + 1)), daemon=True) for i, (how, fam, fresh) in enumerate(jobs)]
    assert len(threads) == 9
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"   # reported, not waited on
    assert not errors, errors


def test_concurrent_workgroup_kernel_plans(gpu, redio, oracle):
    """the three workgroup kernels of the 4096-point LDS image (the Channelizer's, redio_pfb_os_* with one_kernel=True, redio_pfb_pspec_*
    with one_kernel=True): eight threads, each with a plan of its own on a stream of its own, row counts that rise and fall -- a block
    oversampled plan kept and one created fresh every iteration (its destroy runs beside the others' calls), block spectrometers by rows
    and by segments with K = 17 (the partials regrow), a stream of either family fed in twelve pieces, and a plan that set_unfused flips
    between routes 2 and 0 every iteration; every result bit for bit the restatement's"""
    import pfb_os_ref
    import pfb_pspec_ref
    errors = []
    rows_of = [1, 3, 2, 5, 1, 4, 6, 2, 7, 3, 1, 8]   # per iteration: up and down, the largest last
    FIRST = 3

    def same(got, want):
        return got.shape == want.shape and np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32))

    def worker(kind, M, P, K, seed):
        try:
            s = gpu.cuda.Stream()
            with gpu.cuda.stream(s):
                H = M // 2
                h = oracle.synth_f32(seed, 0, M * P)
                if kind == "chan":
                    plan = redio.Channelizer(h, M, P)
                elif kind.startswith("os"):
                    plan = redio.OversampledChannelizer(h, M, P, H, one_kernel=True)
                    assert plan.route == 2 and not plan.is_fused
                else:
                    plan = redio.PolyphaseSpectrum(h, M, P, K, one_kernel=True)
                    assert plan.route == 2 and not plan.is_fused
                    plan.set_split({"spec_rows": 1, "spec_segments": 2}.get(kind, 0))
                if kind in ("os_stream", "spec_stream"):   # one stream in twelve pieces against the one-shot result of the whole
                    window, hop, per = (M * P, H, M) if kind == "os_stream" else (*pfb_pspec_ref.shape(M, P, K), M)
                    lens = [(window - hop if it == 0 else 0) + 5 * rows * hop + 7 * it for it, rows in enumerate(rows_of)]
                    x = oracle.synth_iq(seed, 0, sum(lens))
                    whole = (pfb_os_ref.channelize(x, h, M, P, H, 0, True) if kind == "os_stream" else pfb_pspec_ref.spectrum(x, h, M, P, K, True)).reshape(-1)
                    d = gpu.from_numpy(x).cuda()
                    st = redio.OversampledChannelizerStream(plan) if kind == "os_stream" else redio.Stream(plan)
                    pos = made = 0
                    for it, n in enumerate(lens):
                        got = st(d[pos: pos + n]).cpu().numpy().reshape(-1)
                        pos += n
                        now = (pos - window) // hop + 1 if pos >= window else 0
                        if not (same(got, whole[made * per: now * per]) and st.pending == pos - now * hop):
                            errors.append((kind, it))
                        made = now
                    assert made * per == len(whole) and made >= 5 * sum(rows_of) and plan.route == 2
                    return
                for it, rows in enumerate(rows_of):
                    if kind == "chan":
                        x = oracle.synth_iq(seed + it, 0, M * (P - 1 + rows * 20 + it) + 7 * it)
                        got = plan(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = oracle.pfb_channelizer(x, h, M, P, fused=True)
                    elif kind.startswith("os"):
                        if kind == "os_fresh" and it:
                            plan = redio.OversampledChannelizer(h, M, P, H, one_kernel=True)   # the one before is dropped here
                        if kind == "os_flip":
                            plan.set_unfused(it % 2 == 1)
                            assert plan.route == (0 if it % 2 else 2)
                        units = rows * 20 + it   # up to 171 rows: past a stream's floor, odd and even counts
                        x = oracle.synth_iq(seed + it, 0, (units - 1) * H + M * P + 7 * it % H)
                        got = plan(gpu.from_numpy(x).cuda(), first_row=FIRST + it).cpu().numpy()
                        want = pfb_os_ref.channelize(x, h, M, P, H, FIRST + it, True)
                        assert len(want) == units
                    else:
                        W, Hs = pfb_pspec_ref.shape(M, P, K)
                        x = oracle.synth_iq(seed + it, 0, W + (3 * rows - 1) * Hs + 7 * it)
                        got = plan(gpu.from_numpy(x).cuda()).cpu().numpy()
                        want = pfb_pspec_ref.spectrum(x, h, M, P, K, True)
                        assert len(want) == 3 * rows
                    if not same(got, want):
                        errors.append((kind, it))
        except Exception as e:  # noqa: BLE001
            errors.append((kind, repr(e)))

    jobs = [("chan", 256, 8, 0), ("os_kept", 128, 4, 0), ("os_fresh", 1024, 4, 0), ("spec_rows", 256, 8, 5), ("spec_segments", 128, 4, 17),
            ("os_stream", 512, 8, 0), ("spec_stream", 32, 16, 3), ("os_flip", 256, 4, 0)]
    threads = [threading.Thread(target=worker, args=(*job, 1000 * (i + 1)), daemon=True) for i, job in enumerate(jobs)]
    assert len(threads) <= 9
    for t in threads:
        t.start()
    for t in threads:
        t.join(300)
    assert not any(t.is_alive() for t in threads), "a thread did not finish"   # reported, not waited on
    assert not errors, errors
