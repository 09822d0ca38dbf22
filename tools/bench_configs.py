"""Throughput of the non-headline configs of BASELINE.json on one MI355X (own measurements; bench.py
stays on configs[1]).  usage: python tools/bench_configs.py [c3|c4|fir|fft|fftr|ovsavereal|pspec|pspecu8|pspecreal|pspecrealsplit|pfbpspec|pfbpspecsplit|pfbpspecp2|pfbpspecp2split|ddc|ddcu8|upfirdn|pfbsynth|ddcupfirdn|ddcupfirdnu8|pfbos|pfbosp2|pfbossynth]..."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, libredio_amd as R


def timeit(f, n=50, warm=10, warm_ms=100.0):
    """mean of n launches after `warm` launches AND at least warm_ms of back-to-back work: the chip raises its clock over the first
    50-100 ms of a burst (profiles/r02_clock_probe.txt; bench.py pre-conditions its line the same way, disclosed there), and a line
    timed inside that ramp reads 3-15 % low"""
    import time
    for _ in range(warm): f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while (time.perf_counter() - t0) * 1e3 < warm_ms:
        for _ in range(4): f()
        torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): f()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


which = sys.argv[1:] or ["c4", "fir", "fft"]
n = 1 << 28
if "c4" in which:
    h = R.dsputils.lpf_corrected(1024, 0.45 / 64)
    x = R.synth_iq(0x5EED0004, 0, n)
    plan = R.Channelizer(h)
    out = torch.empty((plan.nrows(n), 64), dtype=torch.complex64, device="cuda")
    ms = timeit(lambda: plan(x, out=out))
    print(f"C4 channelizer 64ch P=16: {ms:.3f} ms  {n/ms/1e6:.1f} GS/s  {16*n/ms/1e6:.0f} GB/s algorithmic ({16*n/ms/1e6/8000:.1%} of 8 TB/s)")
    g = torch.empty((8, plan.nrows(n), 8), dtype=torch.complex64, device="cuda")
    ms = timeit(lambda: plan(x, ngroups=8, out=g))
    print(f"C4 channelizer grouped x8 layout: {ms:.3f} ms  {n/ms/1e6:.1f} GS/s")
if "fir" in which:
    taps = R.dsputils.lpf_corrected(127, 0.08)
    x = R.synth_iq(1, 0, n)
    for d in (5, 1):
        plan = R.Fir(taps, d, fused=True)
        out = torch.empty(plan.nout(n), dtype=torch.complex64, device="cuda")
        ms = timeit(lambda: plan(x, out=out), n=20)
        b = 8 + 8 / d
        print(f"FIR 127 taps /{d}: {ms:.3f} ms  {n/ms/1e6:.1f} GS/s  {b*n/ms/1e6:.0f} GB/s algorithmic ({b*n/ms/1e6/8000:.1%})")
if "fft" in which:
    for nfft in (1024, 64, 256, 4096, 16384, 65536, 2048, 512, 128, 32, 16, 8, 4, 8192, 1000, 100, 1536, 243, 30, 192, 768, 6144, 320, 2560):
        x = R.synth_iq(2, 0, n)[: n // nfft * nfft]
        plan = R.Fft(nfft)
        out = torch.empty_like(x)
        ms = timeit(lambda: plan(x, out=out), n=20 if nfft < 16384 else 5, warm=3)
        print(f"FFT {nfft}: {ms:.3f} ms  {x.numel()/ms/1e6:.1f} GS/s  {16*x.numel()/ms/1e6:.0f} GB/s algorithmic ({16*x.numel()/ms/1e6/8000:.1%})")
if "fftr" in which:
    # the real-input transform of 2^28 real samples against what such a stream costs today: the complex transform of the same size on
    # 2^28 cf32 samples (the widening pass f32 -> cf32 that route also needs is NOT counted: a head start for the old route).  The two
    # are timed alternately, twice each, in this one process; the smaller time of each is printed.
    xr_all = R.synth_f32(3, 0, n)
    xc_all = R.synth_iq(2, 0, n)
    for nfft in (2048, 512, 128, 4096, 1000, 131072):
        rows = n // nfft
        xr, xc = xr_all[: rows * nfft], xc_all[: rows * nfft]
        real, cplx = R.Fftr(nfft), R.Fft(nfft)
        real.reserve(rows)
        outr = torch.empty(rows * (nfft // 2 + 1), dtype=torch.complex64, device="cuda")
        outc = torch.empty_like(xc)
        reps = 20 if nfft < 16384 else 5
        ms_r = ms_c = 1e30
        for _ in range(2):
            ms_r = min(ms_r, timeit(lambda: real(xr, out=outr), n=reps, warm=3))
            ms_c = min(ms_c, timeit(lambda: cplx(xc, out=outc), n=reps, warm=3))
        b = 4 + 8 * (nfft // 2 + 1) / nfft  # algorithmic bytes per real sample: the row read once, the M + 1 bins written once
        ns = rows * nfft
        print(f"FFTR {nfft} ({'fused' if real.is_fused else 'generic'}): {ms_r:.3f} ms  {ns/ms_r/1e6:.1f} real GS/s  {b*ns/ms_r/1e6:.0f} GB/s algorithmic "
              f"({b*ns/ms_r/1e6/8000:.1%} of 8 TB/s) | complex FFT {nfft} on as many cf32 samples: {ms_c:.3f} ms  {ns/ms_c/1e6:.1f} GS/s | "
              f"time per sample real / complex = {ms_r/ms_c:.3f}")
        del real, cplx, outr, outc
if "ovsavereal" in which:
    # overlap-save on 2^28 real samples against what such a stream costs today, timed alternately (twice each; the smaller time is
    # printed) in this one process: (a) redio_ovsave on 2^28 cf32 samples -- a widened real stream, its widening pass NOT counted -- and
    # (b) the direct f32 FIR with the same taps.  Then the generic path at two larger block sizes.
    xr = R.synth_f32(3, 0, n)
    xc = R.synth_iq(2, 0, n)
    for nfft, k in ((2048, 127), (4096, 1025), (65536, 8193)):
        taps = R.dsputils.lpf_corrected(k, 0.02)
        real = R.OverlapSaveReal(taps, nfft)
        real.reserve(n)
        outr = torch.empty(real.nout(n), dtype=torch.float32, device="cuda")
        reps = 10 if real.is_fused else 3
        b = 4 * nfft / real.hop + 4  # algorithmic bytes per output sample
        if not real.is_fused:
            ms_r = min(timeit(lambda: real(xr, out=outr), n=reps, warm=2) for _ in range(2))
            print(f"OVSAVE-REAL {nfft}/{k} (generic): {ms_r:.3f} ms  {n/ms_r/1e6:.1f} real GS/s  {b*outr.numel()/ms_r/1e6:.0f} GB/s algorithmic "
                  f"({b*outr.numel()/ms_r/1e6/8000:.1%} of 8 TB/s)")
            del real, outr
            continue
        cplx, fir = R.OverlapSave(taps, nfft), R.Fir(taps, 1, complex_input=False, fused=True)
        outc = torch.empty(cplx.nout(n), dtype=torch.complex64, device="cuda")
        outf = torch.empty(fir.nout(n), dtype=torch.float32, device="cuda")
        ms_r = ms_c = ms_f = 1e30
        for _ in range(2):
            ms_r = min(ms_r, timeit(lambda: real(xr, out=outr), n=reps, warm=3))
            ms_c = min(ms_c, timeit(lambda: cplx(xc, out=outc), n=reps, warm=3))
            ms_f = min(ms_f, timeit(lambda: fir(xr, out=outf), n=reps, warm=3))
        print(f"OVSAVE-REAL {nfft}/{k} (fused): {ms_r:.3f} ms  {n/ms_r/1e6:.1f} real GS/s  {b*outr.numel()/ms_r/1e6:.0f} GB/s algorithmic "
              f"({b*outr.numel()/ms_r/1e6/8000:.1%} of 8 TB/s) | (a) complex overlap-save {nfft}/{k} on as many cf32 samples: {ms_c:.3f} ms  "
              f"{n/ms_c/1e6:.1f} GS/s | (b) direct f32 FIR {k} taps /1: {ms_f:.3f} ms  {n/ms_f/1e6:.1f} GS/s | "
              f"time per sample real / complex = {ms_r/ms_c:.3f}")
        del real, cplx, fir, outr, outc, outf
if "pspec" in which:
    # the integrated power spectrum of 2^28 cf32 samples against the plain 1024-point transform of the same samples (which writes every
    # spectrum back: 16 B per sample), timed alternately, twice each, in this one process; the smaller time of each is printed.  The bar
    # for the fused size: time per sample below the transform's.  Then N = 4096 on the generic path (no bar: it pays the transform's 16 B
    # and the accumulate pass).
    x = R.synth_iq(2, 0, n)
    fft = R.Fft(1024)
    outc = torch.empty_like(x)
    win = R.dsputils.lpf_corrected(1024, 0.1)
    for nfft, k, step, w, mode, label in ((1024, 16, 1024, None, 0, "auto"), (1024, 1024, 1024, None, 1, "mode 1: a wave per row"),
                                          (1024, 1024, 1024, None, 2, "mode 2: a wave per segment + fold"), (1024, 16, 512, win, 0, "auto, windowed, step 512"),
                                          (4096, 16, 4096, None, 0, "generic")):
        plan = R.PowerSpectrum(nfft, k, step, w)
        plan.set_split(mode)
        plan.reserve(n)
        rows = plan.nrows(n)
        out = torch.empty(rows * nfft, dtype=torch.float32, device="cuda")
        reps = 10 if plan.is_fused else 3
        b = 8 * nfft / step + 4 / k  # algorithmic bytes per input sample
        ms_p = ms_f = 1e30
        for _ in range(2):
            ms_p = min(ms_p, timeit(lambda: plan(x, out=out), n=reps, warm=3))
            ms_f = min(ms_f, timeit(lambda: fft(x, out=outc), n=reps, warm=3))
        print(f"PSPEC {nfft} K={k} step={step} ({label}): {rows} rows  {ms_p:.3f} ms  {n/ms_p/1e6:.1f} GS/s  {b*n/ms_p/1e6:.0f} GB/s algorithmic "
              f"({b*n/ms_p/1e6/8000:.1%} of 8 TB/s) | FFT 1024 on the same samples: {ms_f:.3f} ms  {n/ms_f/1e6:.1f} GS/s | "
              f"time per sample pspec / fft = {ms_p/ms_f:.3f}")
        del plan, out
    del x, outc, fft
if "pspecu8" in which:
    # the integrated power spectrum of 2^28 samples that arrive as 2^29 u8 I/Q bytes (made on the device): (u) redio_pspec_enqueue_u8
    # against (a) redio_pspec_enqueue on the same samples already converted and resident as cf32 and (b) redio_data_to_samples +
    # redio_pspec_enqueue, what a caller without the u8 entry does.  Timed alternately, twice each, in this one process; the smaller
    # time of each is printed.  Algorithmic bytes per sample of (u): 2 N / step + 4 / K.  The bar: u < b on every shape; the target
    # for the fused shapes: u / a <= 1.03.
    from libredio_amd import bitfount as B
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=g)
    x = B.data_to_samples(raw)
    conv = torch.empty(n, dtype=torch.complex64, device="cuda")
    win = R.dsputils.lpf_corrected(1024, 0.1)
    for nfft, k, step, w, mode, label in ((1024, 16, 1024, None, 0, "auto"), (1024, 1024, 1024, None, 2, "mode 2: a wave per segment + fold"),
                                          (1024, 16, 512, win, 0, "auto, windowed, step 512"), (4096, 16, 4096, None, 0, "generic")):
        plan = R.PowerSpectrum(nfft, k, step, w)
        plan.set_split(mode)
        plan.reserve(n)
        plan.reserve_u8(2 * n)
        rows = plan.nrows(n)
        out = torch.empty(rows * nfft, dtype=torch.float32, device="cuda")
        reps = 10 if plan.is_fused else 3
        b = 2 * nfft / step + 4 / k  # algorithmic bytes per input sample
        def two():
            B.data_to_samples(raw, out=conv); plan(conv, out=out)
        ms_u = ms_a = ms_b = 1e30
        for _ in range(2):
            ms_u = min(ms_u, timeit(lambda: plan.u8(raw, out=out), n=reps, warm=3))
            ms_a = min(ms_a, timeit(lambda: plan(x, out=out), n=reps, warm=3))
            ms_b = min(ms_b, timeit(two, n=reps, warm=3))
        print(f"PSPEC-U8 {nfft} K={k} step={step} ({label}): {rows} rows  (u) {ms_u:.3f} ms  {n/ms_u/1e6:.1f} GS/s  {b*n/ms_u/1e6:.0f} GB/s algorithmic "
              f"({b*n/ms_u/1e6/8000:.1%} of 8 TB/s) | (a) cf32 resident: {ms_a:.3f} ms  {n/ms_a/1e6:.1f} GS/s | (b) data_to_samples + cf32: {ms_b:.3f} ms  "
              f"{n/ms_b/1e6:.1f} GS/s | u/a = {ms_u/ms_a:.3f}  u/b = {ms_u/ms_b:.3f}")
        del plan, out
    del raw, x, conv
if "pspecreal" in which:
    # the real-input integrated power spectrum of 2^28 real samples: (r) redio_pspec_real_enqueue against (t) redio_fftr at 2048 on the
    # same samples, which writes every spectrum, (b) what a caller without this plan does -- redio_fftr into a spectra buffer (after a
    # gather / window pass where the shape needs one: a window, or a step redio_fftr_enqueue_strided does not take), then
    # PowerSpectrum(nfft // 2 + 1, K).spectra -- whose rows are compared with (r)'s bit for bit before anything is timed, and (c)
    # PowerSpectrum(1024, K) on 2^28 cf32 samples (informational: time per sample, real against complex).  Timed alternately, twice
    # each, in this one process; the smaller time of each is printed.  Algorithmic bytes per real sample of (r): 4 N / step + 4 B / (K step).
    # The bar: r < b on every shape; the target at step == N on the fused size: r < t.
    x = R.synth_f32(3, 0, n)
    xc = R.synth_iq(2, 0, n)
    fftr_t = R.Fftr(2048)
    spec_t = torch.empty((n // 2048) * 1025, dtype=torch.complex64, device="cuda")
    win2k = R.dsputils.lpf_corrected(2048, 0.1)
    for nfft, k, step, w, mode, label in ((2048, 16, 2048, None, 0, "auto"), (2048, 1024, 2048, None, 1, "mode 1: a wave per row"),
                                          (2048, 1024, 2048, None, 2, "mode 2: a wave per segment + fold"),
                                          (2048, 16, 1024, win2k, 0, "auto, windowed, step 1024"), (2048, 16, 2047, None, 0, "auto, step 2047: 4-byte loads"),
                                          (4096, 16, 4096, None, 0, "auto")):
        nb = nfft // 2 + 1
        plan = R.PowerSpectrumReal(nfft, k, step, w)
        plan.set_split(mode)
        plan.reserve(n)
        rows = plan.nrows(n)
        ntr = rows * k
        out = torch.empty(rows * nb, dtype=torch.float32, device="cuda")
        reps = 10 if plan.is_fused else 3
        b = 4 * nfft / step + 4 * nb / (k * step)  # algorithmic bytes per real sample
        # (b): the parent's route
        fr = R.Fftr(nfft)
        fr.reserve(ntr)
        spec = torch.empty(ntr * nb, dtype=torch.complex64, device="cuda")
        out_b = torch.empty_like(out)
        packs = w is not None or step % 2 == 1
        rowbuf = torch.empty((ntr, nfft), dtype=torch.float32, device="cuda") if packs else None
        wd = torch.from_numpy(w).cuda() if w is not None else None
        try:
            old = R.PowerSpectrum(nb, k)
            old.reserve(n)
        except R.RedioError as e:
            old = None
            print(f"PSPEC-REAL {nfft}: leg (b) cannot be built, PowerSpectrum({nb}, {k}): {e}")
        def route_b():
            if packs:
                frames = x.unfold(0, nfft, step)[:ntr]
                if wd is not None: torch.mul(frames, wd, out=rowbuf)
                else: rowbuf.copy_(frames)
                fr(rowbuf.view(-1), out=spec)
            else:
                fr.strided(x, ntr, step, out=spec)
            old.spectra(spec, out=out_b)
        plan(x, out=out)
        same = None
        if old is not None:
            route_b()
            same = torch.equal(out.view(torch.int32), out_b.view(torch.int32))
            assert same, "leg (b) and leg (r) differ"
        cstep = 1024 * step // nfft if (1024 * step) % nfft == 0 else 1024  # the same overlap on the complex side
        cplx = R.PowerSpectrum(1024, k, cstep, None if w is None else R.dsputils.lpf_corrected(1024, 0.1))
        cplx.reserve(n)
        out_c = torch.empty(cplx.nrows(n) * 1024, dtype=torch.float32, device="cuda")
        ms_r = ms_t = ms_b = ms_c = 1e30
        for _ in range(2):
            ms_r = min(ms_r, timeit(lambda: plan(x, out=out), n=reps, warm=3))
            ms_t = min(ms_t, timeit(lambda: fftr_t(x, out=spec_t), n=reps, warm=3))
            if old is not None: ms_b = min(ms_b, timeit(route_b, n=3, warm=2))
            ms_c = min(ms_c, timeit(lambda: cplx(xc, out=out_c), n=reps, warm=3))
        print(f"PSPEC-REAL {nfft} K={k} step={step} ({label}; {'fused' if plan.is_fused else 'generic'}): {rows} rows  (r) {ms_r:.3f} ms  {n/ms_r/1e6:.1f} real GS/s  "
              f"{b*n/ms_r/1e6:.0f} GB/s algorithmic ({b*n/ms_r/1e6/8000:.1%} of 8 TB/s at {b:.3f} B/sample) | (t) FFTR 2048 on the same samples: {ms_t:.3f} ms | "
              f"(b) fftr + PowerSpectrum({nb}).spectra{' after a gather pass' if packs else ''}: {ms_b:.3f} ms, rows bit-equal: {same} | "
              f"(c) PSPEC 1024 on as many cf32 samples: {ms_c:.3f} ms | r/t = {ms_r/ms_t:.3f}  r/b = {ms_r/ms_b:.3f}  r/c = {ms_r/ms_c:.3f}")
        del plan, out, fr, spec, out_b, rowbuf, old, cplx, out_c
    del x, xc, fftr_t, spec_t
if "pspecrealsplit" in which:
    # the table behind PSPEC_REAL_SPLIT_ROWS (pspec_real_core.h): 2^28 real samples, N = 2048, a wave per row against a wave per segment + fold
    x = R.synth_f32(3, 0, n)
    for k in (32, 64, 128, 256, 512):
        plan = R.PowerSpectrumReal(2048, k)
        plan.reserve(n)
        rows = plan.nrows(n)
        out = torch.empty(rows * 1025, dtype=torch.float32, device="cuda")
        ms = [1e30, 1e30]
        for _ in range(2):
            for mode in (1, 2):
                plan.set_split(mode)
                ms[mode - 1] = min(ms[mode - 1], timeit(lambda: plan(x, out=out), n=10, warm=3))
        print(f"PSPEC-REAL 2048 K={k} ({rows} rows): mode 1 {ms[0]:.3f} ms  mode 2 {ms[1]:.3f} ms")
        del plan, out
    del x
if "pfbpspec" in which:
    # the polyphase spectrometer of 2^28 samples resident in HBM: (n) redio_pfb_pspec_enqueue[_u8] against (a) redio_pfb_enqueue[_u8]
    # alone on the same samples, which writes every channel row, and (b) what a caller without this plan does -- the channelizer into a
    # row buffer as large as the input, then PowerSpectrum(nchan, K).spectra -- whose rows are compared with (n)'s bit for bit before
    # anything is timed.  Timed alternately, twice each, in this one process; the smaller time of each is printed.  Algorithmic bytes
    # per sample of (n): 8 (cf32) or 2 (u8) + 4 / K; of (b): 8 or 2 read + 8 written + 8 read + 4 / K.
    # The bar: n < b on every shape; the target on the fused cf32 shapes: n < a.
    xc = R.synth_iq(0x5EED0004, 0, n)
    xb = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for M, P, k, u8 in ((64, 16, 16, False), (64, 16, 1024, False), (64, 4, 16, False), (64, 16, 16, True), (64, 16, 1024, True), (64, 4, 16, True),
                        (256, 8, 16, False)):
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        plan = R.PolyphaseSpectrum(h, M, P, k)
        plan.reserve(n, u8=u8)
        x = xb if u8 else xc
        rows = plan.nrows(n)
        out = torch.empty(rows * M, dtype=torch.float32, device="cuda")
        chan = R.Channelizer(h, M, P)
        if u8: R.check(R.lib().redio_pfb_reserve_u8(chan._h, 2 * n, 1), "pfb_reserve_u8")
        else: chan.reserve(n)
        crows = torch.empty((chan.nrows(n), M), dtype=torch.complex64, device="cuda")
        old = R.PowerSpectrum(M, k)
        old.reserve(rows * k * M)
        out_b = torch.empty_like(out)
        run_n = (lambda: plan.from_bytes(x, out=out)) if u8 else (lambda: plan(x, out=out))
        run_a = (lambda: chan.from_bytes(x, out=crows)) if u8 else (lambda: chan(x, out=crows))
        def route_b():
            run_a()
            old.spectra(crows.view(-1)[: rows * k * M], out=out_b)
        run_n(); route_b()
        same = torch.equal(out.view(torch.int32), out_b.view(torch.int32))
        assert same, "leg (b) and leg (n) differ"
        reps = 10 if plan.is_fused else 3
        ms_n = ms_a = ms_b = 1e30
        for _ in range(2):
            ms_n = min(ms_n, timeit(run_n, n=reps, warm=3))
            ms_a = min(ms_a, timeit(run_a, n=reps, warm=3))
            ms_b = min(ms_b, timeit(route_b, n=3, warm=2))
        b = (2 if u8 else 8) + 4 / k
        print(f"PFB-PSPEC {M}x{P} K={k} from {'u8' if u8 else 'cf32'} ({'fused' if plan.is_fused else 'generic'}): {rows} rows  (n) {ms_n:.3f} ms  {n/ms_n/1e6:.1f} GS/s  "
              f"{b*n/ms_n/1e6:.0f} GB/s algorithmic ({b*n/ms_n/1e6/8000:.1%} of 8 TB/s at {b:.3f} B/sample) | (a) channelizer alone: {ms_a:.3f} ms | "
              f"(b) channelizer + PowerSpectrum({M}, {k}).spectra: {ms_b:.3f} ms, rows bit-equal: {same} | n/a = {ms_n/ms_a:.3f}  n/b = {ms_n/ms_b:.3f}", flush=True)
        del plan, out, chan, crows, old, out_b
    del xc, xb
if "pfbpspecsplit" in which:
    # the table behind PFBSPEC_SPLIT_WAVES (pfb_pspec_core.h): 2^28 cf32 samples, 64 x 16, a wave per run of whole rows against a wave per
    # run of whole segments + fold.  Waves of mode 1: one per output row from K = 64 up (2 rows per wave at K = 32)
    x = R.synth_iq(0x5EED0004, 0, n)
    h = R.dsputils.lpf_corrected(1024, 0.45 / 64)
    for k in (32, 64, 128, 256, 512, 1024, 2048, 4096):
        plan = R.PolyphaseSpectrum(h, 64, 16, k)
        plan.reserve(n)
        rows = plan.nrows(n)
        out = torch.empty(rows * 64, dtype=torch.float32, device="cuda")
        ms = [1e30, 1e30]
        for _ in range(2):
            for mode in (1, 2):
                plan.set_split(mode)
                ms[mode - 1] = min(ms[mode - 1], timeit(lambda: plan(x, out=out), n=10, warm=3))
        print(f"PFB-PSPEC 64x16 K={k} ({rows} rows, {min(rows, 2048) if k >= 64 else -(-rows // max(2, -(-rows // 2048)))} waves in mode 1): mode 1 {ms[0]:.3f} ms  mode 2 {ms[1]:.3f} ms", flush=True)
        del plan, out
    del x
if "pfbpspecp2" in which:
    # the polyphase spectrometer's workgroup kernel (route 2, REDIO_PFB_PSPEC_BLOCK) on 2^28 samples resident in HBM: (n) the flagged
    # plan against (a) redio_pfb_enqueue[_u8] alone on the same samples, which writes every channel row, and (b) the unflagged plan of
    # the same shape (the generic route), whose rows are compared with (n)'s bit for bit before anything is timed.  Timed alternately,
    # twice each, in this one process; the smaller time of each is printed.  Algorithmic bytes per sample of (n): 8 (cf32) or 2 (u8)
    # + 4 / K; of (b): 8 or 2 read + 8 written + 8 read + 4 / K.  The bar: n < b on every shape; the target from cf32: n < a.
    xc = R.synth_iq(0x5EED0004, 0, n)
    xb = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    for u8 in (False, True):
        for M, P, k in ((32, 16, 16), (128, 8, 16), (256, 8, 16), (256, 16, 16), (512, 8, 16), (1024, 4, 16), (256, 8, 1024)):
            h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
            plan = R.PolyphaseSpectrum(h, M, P, k, one_kernel=True)
            base = R.PolyphaseSpectrum(h, M, P, k)
            assert plan.route == plan.BLOCK and base.route == base.GENERIC
            plan.reserve(n, u8=u8); base.reserve(n, u8=u8)
            x = xb if u8 else xc
            rows = plan.nrows(n)
            out = torch.empty(rows * M, dtype=torch.float32, device="cuda")
            out_b = torch.empty_like(out)
            chan = R.Channelizer(h, M, P)
            if u8: R.check(R.lib().redio_pfb_reserve_u8(chan._h, 2 * n, 1), "pfb_reserve_u8")
            else: chan.reserve(n)
            crows = torch.empty((chan.nrows(n), M), dtype=torch.complex64, device="cuda")
            run_n = (lambda: plan.from_bytes(x, out=out)) if u8 else (lambda: plan(x, out=out))
            run_b = (lambda: base.from_bytes(x, out=out_b)) if u8 else (lambda: base(x, out=out_b))
            run_a = (lambda: chan.from_bytes(x, out=crows)) if u8 else (lambda: chan(x, out=crows))
            run_n(); run_b()
            same = torch.equal(out.view(torch.int32), out_b.view(torch.int32))
            assert same, "leg (b) and leg (n) differ"
            ms_n = ms_a = ms_b = 1e30
            for _ in range(2):
                ms_n = min(ms_n, timeit(run_n, n=10, warm=3))
                ms_a = min(ms_a, timeit(run_a, n=10 if not u8 else 3, warm=3))
                ms_b = min(ms_b, timeit(run_b, n=3, warm=2))
            b = (2 if u8 else 8) + 4 / k
            print(f"PFB-PSPEC-P2 {M}x{P} K={k} from {'u8' if u8 else 'cf32'}: {rows} rows  (n) {ms_n:.3f} ms  {n/ms_n/1e6:.1f} GS/s  "
                  f"{b*n/ms_n/1e6:.0f} GB/s algorithmic ({b*n/ms_n/1e6/8000:.1%} of 8 TB/s at {b:.3f} B/sample) | (a) channelizer alone: {ms_a:.3f} ms | "
                  f"(b) the unflagged plan: {ms_b:.3f} ms, rows bit-equal: {same} | n/a = {ms_n/ms_a:.3f}  n/b = {ms_n/ms_b:.3f}", flush=True)
            del plan, base, out, out_b, chan, crows
    del xc, xb
if "pfbpspecp2split" in which:
    # the table behind PFBSPEC_P2_SPLIT_GROUPS_PER_CU (pfb_pspec_p2_core.h): 2^28 cf32 samples, a stream per run of whole rows
    # against a stream per run of whole segments + fold
    x = R.synth_iq(0x5EED0004, 0, n)
    for M, P in ((256, 8), (1024, 4)):
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        for k in (32, 64, 128, 256, 512, 1024, 2048, 4096):
            plan = R.PolyphaseSpectrum(h, M, P, k, one_kernel=True)
            assert plan.route == plan.BLOCK
            plan.reserve(n)
            rows = plan.nrows(n)
            out = torch.empty(rows * M, dtype=torch.float32, device="cuda")
            ms = [1e30, 1e30]
            for _ in range(2):
                for mode in (1, 2):
                    plan.set_split(mode)
                    ms[mode - 1] = min(ms[mode - 1], timeit(lambda: plan(x, out=out), n=10, warm=3))
            streams = -(-rows // max(-(-64 // k), -(-rows // (4 * torch.cuda.get_device_properties(0).multi_processor_count * max(1, 256 // M)))))
            print(f"PFB-PSPEC-P2 {M}x{P} K={k} ({rows} rows, {streams} streams in mode 1): mode 1 {ms[0]:.3f} ms  mode 2 {ms[1]:.3f} ms", flush=True)
            del plan, out
    del x
if "fftall" in which:
    for nfft in (6, 9, 10, 12, 15, 20, 24, 25, 27, 30, 40, 45, 48, 60, 75, 80, 81, 90, 96, 100, 120, 125, 150, 160, 180, 192, 200, 225, 240, 243, 250, 300, 320, 360, 384, 400, 450, 480, 500, 600, 625, 640, 720, 729, 768, 800, 900, 960, 1000, 1200, 1280, 1440, 1536, 1600, 1800, 1920, 2000, 2187, 2400, 2560, 3072, 3125, 3200, 3600, 3840, 4000, 4800, 5120, 6144, 6400, 6561, 7680, 8000):
        x = R.synth_iq(2, 0, n)[: n // nfft * nfft]
        plan = R.Fft(nfft)
        out = torch.empty_like(x)
        ms = timeit(lambda: plan(x, out=out), n=6, warm=2)
        print(f"FFT {nfft}: {x.numel()/ms/1e6:.1f}")
if "fftnew" in which:
    for nfft in (18, 36, 72, 144, 216, 288, 432, 576, 648, 864, 1080, 1152, 1296, 1500, 1728, 2160, 2304, 2500, 2880, 3000, 3456, 4050, 4320, 4500, 5000, 5400, 5760, 6000, 6250, 6480, 6750, 6912, 7200, 7290, 7500, 7776, 8100):
        x = R.synth_iq(2, 0, n)[: n // nfft * nfft]
        plan = R.Fft(nfft)
        out = torch.empty_like(x)
        ms = timeit(lambda: plan(x, out=out), n=6, warm=2)
        print(f"FFT {nfft}: {x.numel()/ms/1e6:.1f}")
if "fftct" in which:
    for nfft in (48, 60, 120, 200, 240, 360, 480, 500, 600, 720, 729, 800, 960, 1200, 1440, 1920, 2000, 2400, 3125, 3600, 3840, 4000, 4800, 5120, 6400, 7680, 8000):
        x = R.synth_iq(2, 0, n)[: n // nfft * nfft]
        plan = R.Fft(nfft)
        out = torch.empty_like(x)
        ms = timeit(lambda: plan(x, out=out), n=10, warm=2)
        print(f"FFT {nfft}: {ms:.3f} ms  {x.numel()/ms/1e6:.1f} GS/s  ({16*x.numel()/ms/1e6/8000:.1%})")
if "c3" in which or "c3big" in which:
    import time
    nch, frames = 256, (1 << 22) if "c3big" in which else (1 << 20)
    x = torch.stack([R.synth_f32(100 + c, 0, frames) for c in range(nch)])
    for name, mode in (("exact, one launch", R.Src.EXACT), ("fast f32 polyphase", R.Src.FAST), ("exact, per-refill launches", R.Src.EPOCHS)):
        plan = R.Src(nch, 1, mode=mode)
        plan.process(x, 0.02)
        best = 1e9
        for _ in range(5):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            out, used = plan.process(x, 0.02)
            torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
        b = nch * frames * 4 * (1 + 0.02)
        # the binding roofline (report min(HBM, VALU)): EXACT does v_cvt_f64_f32 + v_mul_f64 + v_add_f64 per tap and
        # lane on 1024 SIMDs at 2.4 GHz; FAST does one v_pk_fma_f32 per two taps.  Taps per output: both wings of the stretched filter.
        tab_half, tab_inc = 22438 - 2, 491
        taps_per_out = 2 * int(tab_half / (tab_inc * 0.02)) + 1
        tap_waves = nch * frames * 0.02 * taps_per_out / 64
        # EXACT: issue cost of the tap's instructions measured back to back at two waves per SIMD (tools/valu_rate_f64.hip,
        # profiles/r02_c3_experiments.txt): v_cvt_f64_f32 6.2, v_mul_f64 5.0, v_add_f64 4.6 cycle-equivalents at 2.4 GHz.  The
        # one-launch kernel shares a conversion between the two outputs of a lane (round 3): 6.2 / 2 + 5.0 + 4.6 = 12.7 per tap-wave;
        # the per-refill kernel converts per tap: 13.3 (its measured three-instruction figure).  FAST: one 4-cycle v_pk_fma_f32 per two taps
        cyc = 2 if mode == R.Src.FAST else (12.7 if mode == R.Src.EXACT else 13.3)
        t_valu = tap_waves * cyc / 1024 / 2.4e9
        t_hbm = b / 8e12
        bound = "VALU f64" if mode != R.Src.FAST else "VALU f32"
        print(f"C3 resample 1/50 x{nch} ch, {frames} frames each ({name}): {best*1e3:.2f} ms  {nch*frames/best/1e9:.2f} GS/s  {b/best/1e9:.0f} GB/s algorithmic "
              f"({b/best/8e12:.1%} of 8 TB/s) | rooflines: HBM {t_hbm*1e3:.3f} ms, {bound} {t_valu*1e3:.3f} ms ({taps_per_out} taps/output, {cyc} issue cycles per tap-wave) "
              f"-> binding = {bound if t_valu > t_hbm else 'HBM'}, achieved {max(t_valu, t_hbm)/best:.1%} of it")
if "c5" in which or "c5only" in which:
    for k in ((8193, 127) if "c5" in which else (8193,)):
        taps = R.dsputils.lpf_corrected(k, 0.08)
        x = R.synth_iq(0x5EED0005, 0, n)
        plan = R.OverlapSave(taps, 65536)
        out = torch.empty(plan.nout(n), dtype=torch.complex64, device="cuda")
        ms = timeit(lambda: plan(x, out=out), n=10, warm=3)
        hop = 65536 - k + 1
        b = 8 * 65536 / hop + 8
        print(f"C5 overlap-save N=65536 K={k}: {ms:.3f} ms  {out.numel()/ms/1e6:.1f} GS/s out  {b*out.numel()/ms/1e6:.0f} GB/s algorithmic ({b*out.numel()/ms/1e6/8000:.1%})")
    for nfft, k in (((1024, 127), (1024, 63), (2048, 127), (2048, 513), (8192, 127), (32768, 127), (4096, 127), (4096, 1025), (16384, 127), (16384, 4097)) if "c5" in which else ()):
        taps = R.dsputils.lpf_corrected(k, 0.08)
        x = R.synth_iq(0x5EED0005, 0, n)
        plan = R.OverlapSave(taps, nfft)
        out = torch.empty(plan.nout(n), dtype=torch.complex64, device="cuda")
        ms = timeit(lambda: plan(x, out=out), n=10, warm=3)
        b = 8 * nfft / (nfft - k + 1) + 8
        print(f"overlap-save N={nfft} K={k}: {ms:.3f} ms  {out.numel()/ms/1e6:.1f} GS/s out  {b*out.numel()/ms/1e6:.0f} GB/s algorithmic ({b*out.numel()/ms/1e6/8000:.1%})")
if "hipfft" in which:
    # same-hardware yardstick: the vendor FFT through torch.fft, same sizes, same batch
    for nfft in (1024, 64, 4096, 65536):
        x = R.synth_iq(2, 0, n if nfft != 65536 else 1 << 24).view(-1, nfft)
        out = torch.empty_like(x)
        ms = timeit(lambda: torch.fft.fft(x, dim=1, out=out), n=20, warm=3)
        print(f"vendor FFT (torch.fft -> hipFFT) {nfft}: {ms:.3f} ms  {x.numel()/ms/1e6:.1f} GS/s  ({16*x.numel()/ms/1e6/8000:.1%} of 8 TB/s)")
if "ingest" in which:
    # the u8 front end of the shipped graph and the run-length stage
    from libredio_amd import bitfount as B, kpn_dev as K
    nb = 1 << 29                                            # bytes = 2^28 IQ samples
    raw = torch.randint(0, 256, (nb,), dtype=torch.uint8, device="cuda")
    ns = nb // 2
    ms = timeit(lambda: B.data_to_samples(raw), n=10, warm=2)
    print(f"data_to_samples u8->cf32: {ms:.3f} ms  {ns/ms/1e6:.1f} GS/s  {10*ns/ms/1e6:.0f} GB/s algorithmic ({10*ns/ms/1e6/8000:.1%})")
    ms = timeit(lambda: B.ingest_mag(raw), n=10, warm=2)
    print(f"ingest u8->|x| fused: {ms:.3f} ms  {ns/ms/1e6:.1f} GS/s  {6*ns/ms/1e6:.0f} GB/s algorithmic ({6*ns/ms/1e6/8000:.1%})")
    mag = B.ingest_mag(raw)
    ms = timeit(lambda: B.block_sums(mag, 512), n=10, warm=2)
    print(f"block sums (512, sequential order): {ms:.3f} ms  {ns/ms/1e6:.1f} GS/s  {4*ns/ms/1e6:.0f} GB/s ({4*ns/ms/1e6/8000:.1%})")
    ms = timeit(lambda: B.discretize(mag), n=10, warm=2)
    print(f"discretize (max + threshold): {ms:.3f} ms  {ns/ms/1e6:.1f} GS/s  {(4+4+1)*ns/ms/1e6:.0f} GB/s ({9*ns/ms/1e6/8000:.1%})")
    bits = (torch.rand(ns, device="cuda") > 0.97).to(torch.uint8)   # sparse changes, like a sliced burst
    r = K.Rle()
    ms = timeit(lambda: r.feed(bits), n=10, warm=2)
    print(f"rle (u8 stream, ~6% changes): {ms:.3f} ms  {ns/ms/1e6:.1f} G values/s")
    c = R.synth_f32(5, 0, ns)
    ms = timeit(lambda: K.mul_vecs(mag, c), n=10, warm=2)
    print(f"mul_vecs f32: {ms:.3f} ms  {ns/ms/1e6:.1f} GS/s  {12*ns/ms/1e6:.0f} GB/s ({12*ns/ms/1e6/8000:.1%})")
if "graph" in which:
    # launch-bound: 256 messages of one 1024-point block each, FIR kernel + FFT kernel per message
    import time
    taps = R.dsputils.lpf_corrected(127, 0.08)
    nmsg, n_in = 256, 5120 + 126
    d = R.synth_iq(7, 0, nmsg * n_in).view(nmsg, n_in)
    fir, fft = R.Fir(taps, 5, fused=True), R.Fft(1024)
    y = torch.empty((nmsg, 1024), dtype=torch.complex64, device="cuda"); z = torch.empty_like(y)
    def run():
        for i in range(nmsg):
            fir(d[i], out=y[i]); fft(y[i], out=z[i])
    run(); torch.cuda.synchronize()
    g = R.Graph()
    with g:
        run()
    def wall(f, n=20):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(n): f()
        torch.cuda.synchronize(); return (time.perf_counter() - t0) / n
    a, b = wall(run), wall(g.launch)
    print(f"{2*nmsg} small launches: direct {a*1e3:.2f} ms ({a/nmsg/2*1e6:.1f} us per launch), graph replay {b*1e3:.3f} ms ({b/nmsg/2*1e6:.2f} us per launch)")
if "firshapes" in which:
    # generality of the FIR: specialised shapes vs the direct kernel (any K, D)
    m = 1 << 26
    xc = R.synth_iq(1, 0, m); xr = R.synth_f32(1, 0, m)
    for (k, d, cplx) in ((127, 5, True), (127, 1, True), (127, 3, True), (63, 5, True), (63, 5, False), (127, 1, False), (63, 1, False), (63, 1, True), (64, 1, True), (101, 3, True), (31, 2, True), (255, 10, True), (1023, 1, True), (8193, 1, True)):
        taps = R.dsputils.lpf_corrected(k, 0.4 / d if d > 1 else 0.2)
        plan = R.Fir(taps, d, complex_input=cplx, fused=True)
        x = xc if cplx else xr
        out = torch.empty(plan.nout(m), dtype=x.dtype, device="cuda")
        ms = timeit(lambda: plan(x, out=out), n=40 if k < 1000 else 5, warm=40 if k < 1000 else 2)  # past the clock ramp of a burst (the 2^26-sample launches are 0.1-0.5 ms)
        b = (8 if cplx else 4) * (1 + 1 / d)
        fl = (4 if cplx else 2) * k / d
        # min(HBM, VALU) with the binding one named: the shape's floor is the larger of its HBM time (8 TB/s) and its
        # multiply-add time (157.3 TFLOP/s f32 vector peak)
        t_hbm, t_valu = b * m / 8e12 * 1e3, fl * m / 157.3e12 * 1e3
        bind = "HBM" if t_hbm >= t_valu else "VALU"
        print(f"FIR K={k} D={d} {'cf32' if cplx else 'f32'}: {ms:.3f} ms  {m/ms/1e6:.1f} GS/s  {b*m/ms/1e6/8000:.1%} of HBM roofline, {fl*m/ms/1e9:.1f} TFLOP/s "
              f"({fl*m/ms/1e9/157.3:.1%} of 157.3) -> binding = {bind}, achieved {max(t_hbm, t_valu)/ms:.1%} of it")
if "u8chain" in which:
    # the receiver's format in: u8 I/Q bytes -> data_to_samples -> 127-tap FIR / 5 -> 1024-point FFT, one kernel against two
    from libredio_amd import bitfount as B
    taps = R.dsputils.lpf_corrected(127, 0.08)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=g)
    for fused in (True, False):
        plan = R.Chain(taps, 5, 1024, fused=fused)
        out = torch.empty((plan.nblocks(n), 1024), dtype=torch.complex64, device="cuda")
        ms = timeit(lambda: plan.from_bytes(raw, out=out), n=100, warm=30)
        conv = torch.empty(n, dtype=torch.complex64, device="cuda")
        def two():
            B.data_to_samples(raw, out=conv); plan(conv, out=out)
        ms2 = timeit(two, n=50, warm=10)
        b = 2 + 8 / 5
        print(f"u8 I/Q bytes -> chain ({'fmaf' if fused else 'reference rounding'}), one kernel: {ms:.3f} ms  {n/ms/1e6:.1f} GS/s  {b*n/ms/1e6:.0f} GB/s algorithmic "
              f"({b*n/ms/1e6/8000:.1%} of 8 TB/s at 3.6 B/sample) | conversion kernel + cf32 chain: {ms2:.3f} ms  {n/ms2/1e6:.1f} GS/s")
if "u8c4" in which:
    # the channelizer from the receiver's bytes: one kernel against the conversion kernel + the cf32 channelizer
    from libredio_amd import bitfount as B
    plan = R.Channelizer(R.dsputils.lpf_corrected(1024, 0.45 / 64))
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=g)
    out = torch.empty((plan.nrows(n), 64), dtype=torch.complex64, device="cuda")
    ms = timeit(lambda: plan.from_bytes(raw, out=out), n=50, warm=20)
    conv = torch.empty(n, dtype=torch.complex64, device="cuda")
    def two():
        B.data_to_samples(raw, out=conv); plan(conv, out=out)
    ms2 = timeit(two, n=30, warm=10)
    print(f"u8 I/Q bytes -> C4 channelizer 64ch P=16, one kernel: {ms:.3f} ms  {n/ms/1e6:.1f} GS/s  {10*n/ms/1e6:.0f} GB/s algorithmic ({10*n/ms/1e6/8000:.1%} of 8 TB/s at 10 B/sample)"
          f" | conversion kernel + cf32 channelizer: {ms2:.3f} ms  {n/ms2/1e6:.1f} GS/s")
if "srcgen" in which:
    # the general (non-uniform phase) resampler path: arbitrary ratios, one launch per buffer refill
    import time
    nch, frames = 64, 1 << 18
    x = torch.stack([R.synth_f32(100 + c, 0, frames) for c in range(nch)])
    for ratio in (0.02, 0.0213, 0.5, 48000 / 44100, 2.0, 1.5, 0.3):
        for name, mode in (("default", R.Src.EXACT), ("per-refill general kernel", R.Src.EPOCHS)):
            plan = R.Src(nch, 1, mode=mode)
            plan.process(x, ratio)
            best = 1e9
            for _ in range(3):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                out, used = plan.process(x, ratio)
                torch.cuda.synchronize(); best = min(best, time.perf_counter() - t0)
            per, gen = plan.path_counts()
            print(f"resample ratio {ratio:.5f} x{nch} ch, {frames} frames ({name}; epochs periodic/general {per}/{gen}): {best*1e3:.2f} ms  "
                  f"{nch*used/best/1e9:.3f} GS/s in, {best*1e9/(nch*used):.3f} ns per input frame, {out.shape[1]} out per channel")
if "srcsmall" in which:
    # the reference's calling pattern (samplerate.rs:59-87: one message per src_process call): small messages x 256 channels at 1/50, per-call time on
    # the stream and on the host clock -- catches a per-call cost that does not scale with the message (round 4's image rebuild; advisor, round 4)
    import time
    nch = 256
    for frames in (1024, 4096, 16384, 65536):
        x = torch.stack([R.synth_f32(100 + c, 0, frames) for c in range(nch)])
        for name, mode in (("exact", R.Src.EXACT), ("fast", R.Src.FAST)):
            plan = R.Src(nch, 1, mode=mode)
            for _ in range(20): plan.process(x, 0.02)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter(); e0.record()
            for _ in range(200): plan.process(x, 0.02)
            e1.record(); torch.cuda.synchronize(); wall = (time.perf_counter() - t0) / 200
            print(f"resample 1/50 x{nch} ch, {frames} frames per message ({name}): {e0.elapsed_time(e1) / 200 * 1e3:.1f} us per call on the stream, "
                  f"{wall * 1e6:.1f} us wall, {nch * frames / wall / 1e9:.2f} GS/s")
if "c4gen" in which:
    for M, P in ((64, 16), (32, 16), (128, 16), (256, 16), (256, 8), (128, 8), (32, 4), (512, 8), (1024, 4), (64, 12)):
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        x = R.synth_iq(0x5EED0004, 0, n)
        plan = R.Channelizer(h, M, P)
        out = torch.empty((plan.nrows(n), M), dtype=torch.complex64, device="cuda")
        ms = timeit(lambda: plan(x, out=out), n=10, warm=3)
        print(f"channelizer M={M} P={P}: {ms:.3f} ms  {n/ms/1e6:.1f} GS/s  ({16*n/ms/1e6/8000:.1%} of 8 TB/s)")
if "chains" in which:
    for (k, d) in ((127, 5), (63, 5), (127, 3), (127, 1), (63, 1), (64, 4)):
        taps = R.dsputils.lpf_corrected(k, 0.4 / max(d, 2))
        m = 1 << 27
        x = R.synth_iq(2, 0, m)
        plan = R.Chain(taps, d, 1024, fused=True)
        out = torch.empty((plan.nblocks(m), 1024), dtype=torch.complex64, device="cuda")
        ms = timeit(lambda: plan(x, out), n=10, warm=3)
        b = 8 + 8 / d
        print(f"chain K={k} D={d} -> FFT 1024 ({'one kernel' if plan.is_fused else 'two kernels'}): {ms:.3f} ms  {m/ms/1e6:.1f} GS/s  ({b*m/ms/1e6/8000:.1%} of 8 TB/s)")
if "trigger" in which:
    # bitfount::trigger on a long capture: bursts every ~2^20 samples on a noise floor (block sums on the device,
    # the state machine on the host, triggered blocks gathered on the device)
    import time
    from libredio_amd import bitfount as B
    ns = 1 << 27
    mag = torch.rand(ns, device="cuda") * 0.05
    idx = torch.arange(ns, device="cuda")
    mag += ((idx % (1 << 20)) < 60000).float() * 0.8
    blocks = mag.view(-1, 512)
    trig = B.Trigger()
    trig.feed(blocks[:4096])
    torch.cuda.synchronize(); t0 = time.perf_counter()
    bufs = trig.feed(blocks)
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    print(f"trigger over {ns} samples ({blocks.shape[0]} blocks): {dt*1e3:.2f} ms  {ns/dt/1e9:.1f} GS/s, {len(bufs)} buffers emitted, {sum(b.numel() for b in bufs)} samples kept")
if "upfirdn" in which:
    # the rational resampler (redio_upfirdn_*: up U, FIR, down D as a polyphase FIR over the original samples) on 2^28 cf32 input samples,
    # fused fold, against the composition it replaces, timed alternately (twice each, the smaller time printed) in this one process:
    # zero-stuff into a U-times buffer (a strided copy into a buffer zeroed ONCE outside the timing: a head start for the old route),
    # then redio_fir(K, D).  Share of 8 TB/s on the algorithmic bytes, 8 + 8 D / U per output.  160/147 would need a 320 GiB
    # zero-stuffed buffer at 2^28 samples: its ratio is taken at 2^22 samples, both sides, and its own time at 2^28 as well.
    x = R.synth_iq(1, 0, n)
    for U, D, K in ((2, 1, 63), (3, 2, 96), (2, 3, 63), (4, 5, 127), (1, 5, 127), (160, 147, 3841)):
        taps = R.dsputils.lpf_corrected(K, 0.4 / max(U, D))
        plan = R.Upfirdn(taps, U, D, complex_input=True, fused=True)
        fir = R.Fir(taps, D, fused=True)
        out = torch.empty(plan.nout(n), dtype=torch.complex64, device="cuda")
        b = 8 + 8 * D / U
        ms = timeit(lambda: plan(x, out=out), n=10, warm=3)
        nc = n if U <= 4 else 1 << 22  # the samples of the comparison
        xc = x[:nc]
        z = torch.zeros(nc * U, dtype=torch.complex64, device="cuda") if U > 1 else None
        outc = out[: plan.nout(nc)]

        def old():
            if U > 1:
                z[::U].copy_(xc)
                fir(z, out=outc)
            else:
                fir(xc, out=outc)
        ms_new = ms_old = 1e30
        for _ in range(2):
            ms_new = min(ms_new, timeit(lambda: plan(xc, out=outc), n=10, warm=3))
            ms_old = min(ms_old, timeit(old, n=5, warm=2))
        what = "zero-stuff + fir" if U > 1 else "fir alone (no bar)"
        print(f"UPFIRDN {U}/{D} {K} taps (route {plan.route}, U'={plan.period_out} D'={plan.period_in} Wp={plan.window}): {ms:.3f} ms  "
              f"{out.numel()/ms/1e6:.1f} GS/s out  {b*out.numel()/ms/1e6:.0f} GB/s algorithmic ({b*out.numel()/ms/1e6/8000:.1%} of 8 TB/s) | "
              f"at {nc} samples: {ms_new:.3f} ms against {what}: {ms_old:.3f} ms, resampler / composition = {ms_new/ms_old:.3f}")
        del plan, fir, out, outc, z
if "pfbsynth" in which:
    # the synthesis filterbank (redio_pfb_synth_*: inverse transform per row, then the channelizer's branch filter) on 2^28 channel values in,
    # fused fold: 64 x 16 and 64 x 4 on the wave kernel (route 1) and the same plans through set_unfused (route 0: the inverse transform into
    # scratch, then the branch pass), 256 x 8 on route 0; and the Channelizer of the same prototype on as many samples.  The variants of a
    # shape are timed alternately (twice each, the smaller time printed) in this one process; the two routes' outputs are compared bit for bit.
    # Share of 8 TB/s on 16 B per sample (8 read + 8 written: route 1's traffic; route 0 moves 32).
    x = R.synth_iq(0x5EED0004, 0, n)
    for M, P in ((64, 16), (64, 4), (256, 8)):
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        plan, two, ana = R.Synthesizer(h, M, P, fused=True), R.Synthesizer(h, M, P, fused=True), R.Channelizer(h, M, P, fused=True)
        two.set_unfused(True)
        two.reserve(n)
        out, out2 = (torch.empty(plan.nout(n), dtype=torch.complex64, device="cuda") for _ in range(2))
        rows = torch.empty((ana.nrows(n), M), dtype=torch.complex64, device="cuda")
        ms = {}
        legs = {"synth": lambda: plan(x, out=out), "two-pass": lambda: two(x, out=out2), "channelizer": lambda: ana(x, out=rows)}
        if plan.route == 0:
            del legs["two-pass"]
        for _ in range(2):
            for name, f in legs.items():
                ms[name] = min(ms.get(name, 1e30), timeit(f, n=10, warm=3))
        line = (f"PFBSYNTH {M}ch P={P} (route {plan.route}): {ms['synth']:.3f} ms  {n/ms['synth']/1e6:.1f} GS/s  ({16*n/ms['synth']/1e6/8000:.1%} of 8 TB/s on 16 B/sample)")
        if plan.route == 1:
            same = torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(out2).view(torch.int32))
            line += f" | set_unfused (route {two.route}): {ms['two-pass']:.3f} ms, route 1 / route 0 = {ms['synth']/ms['two-pass']:.3f}, outputs bit-equal: {same}"
        line += f" | Channelizer on as many samples: {ms['channelizer']:.3f} ms, synthesizer / channelizer = {ms['synth']/ms['channelizer']:.3f}"
        print(line)
        del plan, two, ana, out, out2, rows
if "ddc" in which or "ddcu8" in which:
    # the tuner (redio_ddc_*: oscillator mix fused into the FIR tile load) on 2^28 samples against the route it replaces, timed alternately
    # (twice each, the smaller time printed) in this one process: (a) redio_mul_c32 on a PRE-MATERIALISED oscillator stream (its
    # generation is not counted: a head start for the old route) + redio_fir_enqueue -- for u8 also + redio_data_to_samples -- and
    # (b) redio_fir_enqueue alone (no mix at all; on the complex /5 and /1 shapes that call runs the chain-form data path, which the
    # tuner does not have).  Share of 8 TB/s on the algorithmic bytes: 8 + 8/D per input sample from cf32, 2 + 8/D from u8.
    from libredio_amd.plans import _dev_ptr, current_stream
    x = R.synth_iq(1, 0, n)
    for leg in [l for l in ("ddc", "ddcu8") if l in which]:
        u8 = leg == "ddcu8"
        raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda") if u8 else None
        mixed, conv = torch.empty_like(x), (torch.empty_like(x) if u8 else None)
        for k, d in ((127, 5), (63, 5), (63, 1), (31, 2), (255, 10)):
            taps = R.dsputils.lpf_corrected(k, 0.4 / max(d, 2))
            fir = R.Fir(taps, d, fused=True)
            out = torch.empty(fir.nout(n), dtype=torch.complex64, device="cuda")
            per = {}
            for period in (24, 65536):
                w = R.dsputils.osc_table(-5, 24) if period == 24 else R.dsputils.osc_table(1, 65536)
                plan = R.Ddc(w, taps, d, fused=True)
                osc = torch.from_numpy(w).cuda().repeat((n + period - 1) // period)[:n].contiguous()

                def old():
                    src = x
                    if u8:
                        R.check(R.lib().redio_data_to_samples(_dev_ptr(raw), 2 * n, _dev_ptr(conv), current_stream()), "data_to_samples")
                        src = conv
                    R.check(R.lib().redio_mul_c32(_dev_ptr(src), _dev_ptr(osc), _dev_ptr(mixed), n, current_stream()), "mul_c32")
                    fir(mixed, out=out)
                new = (lambda: plan.from_bytes(raw, out=out)) if u8 else (lambda: plan(x, out=out))
                ms = ms_old = ms_fir = 1e30
                for _ in range(2):
                    ms = min(ms, timeit(new, n=20, warm=3))
                    ms_old = min(ms_old, timeit(old, n=10, warm=3))
                    ms_fir = min(ms_fir, timeit(lambda: fir(x, out=out), n=20, warm=3))
                b = (2 if u8 else 8) + 8 / d
                per[period] = ms
                print(f"{'DDC-U8' if u8 else 'DDC'} {k} taps /{d} period {period} (route {plan.route}): {ms:.3f} ms  {n/ms/1e6:.1f} GS/s  {b*n/ms/1e6:.0f} GB/s algorithmic "
                      f"({b*n/ms/1e6/8000:.1%} of 8 TB/s) | (a) {'data_to_samples + ' if u8 else ''}mul_c32 + fir: {ms_old:.3f} ms, tuner / (a) = {ms/ms_old:.3f} | "
                      f"(b) fir alone: {ms_fir:.3f} ms, tuner / (b) = {ms/ms_fir:.3f}")
                del plan, osc
            print(f"{'DDC-U8' if u8 else 'DDC'} {k} taps /{d}: period 65536 / period 24 = {per[65536]/per[24]:.3f}")
            del fir, out
        del raw, mixed, conv
if "ddcupfirdn" in which or "ddcupfirdnu8" in which:
    # the tuned resampler (redio_ddc_upfirdn_*: oscillator mix fused into the resampler's tile load) on 2^28 input samples, fused fold,
    # against the route it replaces, timed alternately (twice each, the smaller time printed) in this one process: (a) redio_mul_c32 on a
    # PRE-MATERIALISED oscillator stream (its generation is not counted: a head start for the old route) + redio_upfirdn_enqueue -- for
    # u8 also + redio_data_to_samples in front -- after the two outputs were compared bit for bit, and (b) redio_upfirdn_enqueue alone on
    # already-mixed samples (no mix at all: no bar).  Share of 8 TB/s on the algorithmic bytes per OUTPUT: 8 + 8 D / U from cf32,
    # 8 + 2 D / U from u8.  160/147 (route 2) is compared at 2^22 samples, both sides, as the `upfirdn` leg does; its own time at 2^28 too.
    from libredio_amd.plans import _dev_ptr, current_stream
    x = R.synth_iq(1, 0, n)
    for leg in [l for l in ("ddcupfirdn", "ddcupfirdnu8") if l in which]:
        u8 = leg == "ddcupfirdnu8"
        name = "DDCUPFIRDN-U8" if u8 else "DDCUPFIRDN"
        raw = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda") if u8 else None
        mixed, conv = torch.empty_like(x), (torch.empty_like(x) if u8 else None)
        for U, D, K in ((2, 1, 63), (3, 2, 96), (2, 3, 63), (4, 5, 127), (160, 147, 3841)):
            taps = R.dsputils.lpf_corrected(K, 0.4 / max(U, D))
            res = R.Upfirdn(taps, U, D, complex_input=True, fused=True)
            out, out_old = (torch.empty(res.nout(n), dtype=torch.complex64, device="cuda") for _ in range(2))
            nc = n if U <= 4 else 1 << 22  # the samples of the comparison
            outc, outc_old = out[: res.nout(nc)], out_old[: res.nout(nc)]
            per = {}
            for period in (24, 65536):
                w = R.dsputils.osc_table(-5, 24) if period == 24 else R.dsputils.osc_table(1, 65536)
                plan = R.DdcUpfirdn(w, taps, U, D, fused=True)
                osc = torch.from_numpy(w).cuda().repeat((nc + period - 1) // period)[:nc].contiguous()

                def old():
                    src = x[:nc]
                    if u8:
                        R.check(R.lib().redio_data_to_samples(_dev_ptr(raw), 2 * nc, _dev_ptr(conv), current_stream()), "data_to_samples")
                        src = conv[:nc]
                    R.check(R.lib().redio_mul_c32(_dev_ptr(src), _dev_ptr(osc), _dev_ptr(mixed), nc, current_stream()), "mul_c32")
                    res(mixed[:nc], out=outc_old)
                new_c = (lambda: plan.from_bytes(raw[: 2 * nc], out=outc)) if u8 else (lambda: plan(x[:nc], out=outc))
                new = (lambda: plan.from_bytes(raw, out=out)) if u8 else (lambda: plan(x, out=out))
                old(); new_c()
                torch.cuda.synchronize()
                assert torch.equal(torch.view_as_real(outc).view(torch.int32), torch.view_as_real(outc_old).view(torch.int32)), "plan and composition differ"
                ms = timeit(new, n=10, warm=3) if nc != n else 1e30
                ms_new = ms_old = ms_res = 1e30
                for _ in range(2):
                    ms_new = min(ms_new, timeit(new_c, n=10, warm=3))
                    ms_old = min(ms_old, timeit(old, n=5, warm=2))
                    ms_res = min(ms_res, timeit(lambda: res(mixed[:nc], out=outc_old), n=10, warm=3))
                if nc == n:
                    ms = ms_new
                b = 8 + (2 if u8 else 8) * D / U
                per[period] = ms
                print(f"{name} {U}/{D} {K} taps period {period} (route {plan.route}, U'={plan.period_out} D'={plan.period_in} Wp={plan.window}): {ms:.3f} ms  "
                      f"{out.numel()/ms/1e6:.1f} GS/s out  {b*out.numel()/ms/1e6:.0f} GB/s algorithmic ({b*out.numel()/ms/1e6/8000:.1%} of 8 TB/s) | at {nc} samples, "
                      f"outputs bit-equal: {ms_new:.3f} ms against (a) {'data_to_samples + ' if u8 else ''}mul_c32 + upfirdn: {ms_old:.3f} ms, plan / (a) = {ms_new/ms_old:.3f} | "
                      f"(b) upfirdn alone: {ms_res:.3f} ms, plan / (b) = {ms_new/ms_res:.3f}")
                del plan, osc
            print(f"{name} {U}/{D} {K} taps: period 65536 / period 24 = {per[65536]/per[24]:.3f}")
            del res, out, out_old, outc, outc_old
        del raw, mixed, conv
if "pfbos" in which:
    # the oversampled channelizer (redio_pfb_os_*: a row of nchan channels every hop samples, shifted, transformed) on 2^28 input samples, fused
    # fold: 64 x 16 and 64 x 4 at hop 32 on the wave kernel (route 1) and the same plans through set_unfused (route 0: the branch pass into
    # scratch, then the forward transform), 64 x 16 at hop 16 and 256 x 8 at hop 128 on route 0; and the Channelizer of the same prototype on
    # the same input.  The variants of a shape are timed alternately (twice each, the smaller time printed) in this one process; the two
    # routes' outputs are compared bit for bit.  Share of 8 TB/s on 8 + 8 M / H bytes per input sample (read once, every row written once).
    # The bytes say time per output row / the Channelizer's time per output row = (8 H / M + 8) / 16: 0.75 at hop M / 2.
    x = R.synth_iq(0x5EED0004, 0, n)
    for M, P, H in ((64, 16, 32), (64, 4, 32), (64, 16, 16), (256, 8, 128)):
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        plan, two, ana = R.OversampledChannelizer(h, M, P, H, fused=True), R.OversampledChannelizer(h, M, P, H, fused=True), R.Channelizer(h, M, P, fused=True)
        two.set_unfused(True)
        two.reserve(n)
        plan.reserve(n)
        nr = plan.nrows(n)
        out = torch.empty(nr * M, dtype=torch.complex64, device="cuda")
        out2 = torch.empty(nr * M, dtype=torch.complex64, device="cuda") if plan.route == 1 else None
        rows = torch.empty((ana.nrows(n), M), dtype=torch.complex64, device="cuda")
        ms = {}
        legs = {"os": lambda: plan(x, first_row=1, out=out), "two-pass": lambda: two(x, first_row=1, out=out2), "channelizer": lambda: ana(x, out=rows)}
        if plan.route == 0:
            del legs["two-pass"]
        for _ in range(2):
            for name, f in legs.items():
                ms[name] = min(ms.get(name, 1e30), timeit(f, n=10, warm=3))
        b = 8 + 8 * M / H
        per_row = (ms["os"] / nr) / (ms["channelizer"] / ana.nrows(n))
        line = (f"PFBOS {M}ch P={P} hop {H} (route {plan.route}): {ms['os']:.3f} ms  {n/ms['os']/1e6:.1f} GS/s in  {b*n/ms['os']/1e6:.0f} GB/s algorithmic "
                f"({b*n/ms['os']/1e6/8000:.1%} of 8 TB/s on {b:.0f} B/sample)")
        if plan.route == 1:
            same = torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(out2).view(torch.int32))
            line += f" | set_unfused (route {two.route}): {ms['two-pass']:.3f} ms, route 1 / route 0 = {ms['os']/ms['two-pass']:.3f}, outputs bit-equal: {same}"
        line += (f" | Channelizer on the same input: {ms['channelizer']:.3f} ms; time per output row, oversampled / Channelizer = {per_row:.3f} "
                 f"(bytes model {(8 * H / M + 8) / 16:.3f})")
        print(line)
        del plan, two, ana, out, out2, rows
if "pfbosp2" in which:
    # the oversampled channelizer's workgroup kernel (route 2, REDIO_PFB_OS_BLOCK) on 2^28 input samples, fused fold, hop M / 2: the flagged
    # plan, the same plan through set_unfused (route 0, reserved: the branch pass into scratch, then the forward transform) and the
    # Channelizer of the same prototype (pfb_p2_kernel) on the same input.  The three are timed alternately (twice each, the smaller time
    # printed) in this one process; the two routes' outputs are compared bit for bit.  Share of 8 TB/s on 24 B per input sample (read
    # once, a row of M channels written every M / 2 samples).  The bytes say time per output row / the Channelizer's = (8 H / M + 8) / 16 = 0.75.
    x = R.synth_iq(0x5EED0004, 0, n)
    for M, P in ((32, 16), (128, 8), (256, 8), (256, 16), (512, 8), (1024, 4)):
        H = M // 2
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        plan, two, ana = R.OversampledChannelizer(h, M, P, H, fused=True, one_kernel=True), R.OversampledChannelizer(h, M, P, H, fused=True, one_kernel=True), R.Channelizer(h, M, P, fused=True)
        assert plan.route == 2
        two.set_unfused(True)
        two.reserve(n)
        nr = plan.nrows(n)
        out = torch.empty(nr * M, dtype=torch.complex64, device="cuda")
        out2 = torch.empty(nr * M, dtype=torch.complex64, device="cuda")
        rows = torch.empty((ana.nrows(n), M), dtype=torch.complex64, device="cuda")
        ms = {}
        legs = {"block": lambda: plan(x, first_row=1, out=out), "two-pass": lambda: two(x, first_row=1, out=out2), "channelizer": lambda: ana(x, out=rows)}
        for _ in range(2):
            for name, f in legs.items():
                ms[name] = min(ms.get(name, 1e30), timeit(f, n=10, warm=3))
        same = torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(out2).view(torch.int32))
        per_row = (ms["block"] / nr) / (ms["channelizer"] / ana.nrows(n))
        print(f"PFBOSP2 {M}ch P={P} hop {H} (route {plan.route}): {ms['block']:.3f} ms  {n/ms['block']/1e6:.1f} GS/s in  {24*n/ms['block']/1e6:.0f} GB/s algorithmic "
              f"({24*n/ms['block']/1e6/8000:.1%} of 8 TB/s on 24 B/sample) | set_unfused (route {two.route}): {ms['two-pass']:.3f} ms, route 2 / route 0 = "
              f"{ms['block']/ms['two-pass']:.3f}, outputs bit-equal: {same} | Channelizer on the same input: {ms['channelizer']:.3f} ms; time per output row, "
              f"oversampled / Channelizer = {per_row:.3f} (bytes model 0.750)", flush=True)
        del plan, two, ana, out, out2, rows
if "pfbossynth" in which:
    # the oversampled synthesis bank (redio_pfb_os_synth_*: inverse transform per row, then the weighted overlap-add at hop H) on 2^28 channel
    # values in, fused fold: 64 x 16 and 64 x 4 at hop 32 on the wave kernel (route 1) and the same plans through set_unfused (route 0: the
    # inverse transform into scratch, then the overlap-add pass), 64 x 16 at hop 16 and 256 x 8 at hop 128 on route 0; and the Synthesizer of
    # the same prototype on as many values.  The variants of a shape are timed alternately (twice each, the smaller time printed) in this one
    # process; the two routes' outputs are compared bit for bit.  Share of 8 TB/s on 8 + 8 H / M bytes per channel value (read once, every
    # sample written once).  The bytes say time per value / the Synthesizer's = (8 + 8 H / M) / 16: 0.75 at hop M / 2.
    x = R.synth_iq(0x5EED0004, 0, n)
    for M, P, H in ((64, 16, 32), (64, 4, 32), (64, 16, 16), (256, 8, 128)):
        h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
        plan, two, syn = R.OversampledSynthesizer(h, M, P, H, fused=True), R.OversampledSynthesizer(h, M, P, H, fused=True), R.Synthesizer(h, M, P, fused=True)
        two.set_unfused(True)
        two.reserve(n)
        plan.reserve(n)
        syn.reserve(n)
        no = plan.nout(n)
        out = torch.empty(no, dtype=torch.complex64, device="cuda")
        out2 = torch.empty(no, dtype=torch.complex64, device="cuda") if plan.route == 1 else None
        outs = torch.empty(syn.nout(n), dtype=torch.complex64, device="cuda")
        ms = {}
        legs = {"os": lambda: plan(x, first_row=1, out=out), "two-pass": lambda: two(x, first_row=1, out=out2), "synthesizer": lambda: syn(x, out=outs)}
        if plan.route == 0:
            del legs["two-pass"]
        for _ in range(2):
            for name, f in legs.items():
                ms[name] = min(ms.get(name, 1e30), timeit(f, n=10, warm=3))
        b = 8 + 8 * H / M
        line = (f"PFBOSSYNTH {M}ch P={P} hop {H} (route {plan.route}): {ms['os']:.3f} ms  {n/ms['os']/1e6:.1f} GS/s in  {b*n/ms['os']/1e6:.0f} GB/s algorithmic "
                f"({b*n/ms['os']/1e6/8000:.1%} of 8 TB/s on {b:.0f} B/value)")
        if plan.route == 1:
            same = torch.equal(torch.view_as_real(out).view(torch.int32), torch.view_as_real(out2).view(torch.int32))
            line += f" | set_unfused (route {two.route}): {ms['two-pass']:.3f} ms, route 1 / route 0 = {ms['os']/ms['two-pass']:.3f}, outputs bit-equal: {same}"
        line += (f" | Synthesizer on as many values (route {syn.route}): {ms['synthesizer']:.3f} ms; time per value, oversampled / Synthesizer = "
                 f"{ms['os']/ms['synthesizer']:.3f} (bytes model {(8 + 8 * H / M) / 16:.3f})")
        print(line)
        del plan, two, syn, out, out2, outs
