"""redio_src_enqueue: redio_src_process(..., end_of_input = 0) in stream order.  Same outputs, counts and carried state as the oracle
(oracle/oracle_src.c) and as a twin handle driven through redio_src_process, for every path; a uniform-phase call (constant ratio,
integer 1/ratio, samplerate.rs:59-87 at C3's 0.02) whose tables exist only launches: the counters of redio_src_enqueue_counts say
which calls waited for the stream."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = np.uint32(0x7FC0DEAD)
R441 = 48000 / 44100


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cap_of(ratio, m):
    return int(ratio * m + 1.0)


def _fast_bound(oracle, ratio, xmax, conv=1):
    # tests/test_gpu_resample.py: each of the K products carries one f32 tap rounding and the f32 sum at most K roundings
    tab, half, inc = oracle.src_table(conv)
    pos = np.arange(0.0, half, inc * ratio)
    K = 2 * len(pos)
    sum_h = 2 * ratio * np.abs(np.interp(pos, np.arange(half + 2), tab.astype(np.float64))).sum()
    return (K + 1) * 2.0 ** -24 * max(sum_h, 1.0) * xmax


def cuts_of(seg):
    c = [0]
    for m in seg:
        c.append(c[-1] + m)
    return c


@pytest.mark.parametrize("nch", [1, 3, 70])
@pytest.mark.parametrize("seg", [[6000], [1000, 2500, 1, 2499], [37] * 40])
@pytest.mark.parametrize("ratio,conv", [(0.02, 1), (0.5, 1), (1.0, 1), (1 / 256, 2)])
def test_bits_counts_and_state_without_host_sync(gpu, redio, oracle, ratio, conv, seg, nch):
    if ratio < 0.02:
        seg = [50 * m for m in seg]
    cuts = cuts_of(seg)
    n = cuts[-1]
    x = np.stack([oracle.synth_f32(1300 + c, 0, n) for c in range(nch)])
    d = gpu.from_numpy(x).cuda()
    plan, twin = redio.Src(nch, conv), redio.Src(nch, conv)
    got = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):       # back to back: nothing here waits for the device
        got.append(plan.enqueue(d[:, lo:hi], ratio))
    gpu.cuda.synchronize()
    refs = [oracle.Resampler(conv) for _ in range(nch)]
    for (out, used, gen), lo, hi in zip(got, cuts[:-1], cuts[1:]):
        a = out.cpu().numpy()
        assert a.shape == (nch, gen)
        for c in range(nch):
            err, want, wused = refs[c].process(x[c, lo:hi], ratio, cap_of(ratio, hi - lo))
            assert err == 0 and (used, gen) == (wused, len(want)), (c, lo, hi)
            assert np.array_equal(bits(a[c]), bits(want)), (c, lo, hi)
        b, ub = twin.process(d[:, lo:hi].contiguous(), ratio)
        assert ub == used and b.shape == a.shape and np.array_equal(bits(a), bits(b.cpu().numpy())), (lo, hi)
    q, s = plan.enqueue_counts()
    assert q + s == len(seg) and s >= 1           # the first call builds the tables


@pytest.mark.parametrize("nch", [1, 256])
@pytest.mark.parametrize("mode", ["EXACT", "FAST"])
def test_uniform_calls_are_queued_after_the_first(gpu, redio, oracle, nch, mode):
    ratio, m = 0.02, 4096
    x = gpu.empty((nch, 33 * m), dtype=gpu.float32, device="cuda")
    for c in range(nch):
        x[c] = redio.synth_f32(400 + c, 0, 33 * m)
    plan = redio.Src(nch, 1, mode=getattr(redio.Src, mode))
    out = gpu.empty((nch, cap_of(ratio, m)), dtype=gpu.float32, device="cuda")
    plan.enqueue(x[:, :m], ratio, out=out)
    q0, s0 = plan.enqueue_counts()
    assert (q0, s0) == (0, 1)
    total = 0
    for i in range(1, 33):
        _, used, gen = plan.enqueue(x[:, i * m:(i + 1) * m], ratio, out=out)
        assert used == m
        total += gen
    q, s = plan.enqueue_counts()
    gpu.cuda.synchronize()
    assert s == s0, "a uniform-phase call with cached tables synchronised"
    assert q == q0 + 32
    assert abs(total - 32 * m * ratio) <= 2


@pytest.mark.parametrize("nch", [1, 256])
def test_non_integer_step_synchronises_and_matches(gpu, redio, oracle, nch):
    m, nmsg = 4096, 9
    check = sorted({0, nch - 1})
    x = np.stack([oracle.synth_f32(600 + c, 0, nmsg * m) for c in range(nch)])
    d = gpu.from_numpy(x).cuda()
    plan = redio.Src(nch, 1)
    refs = {c: oracle.Resampler(1) for c in check}
    for i in range(nmsg):
        out, used, gen = plan.enqueue(d[:, i * m:(i + 1) * m], R441)
        a = out.cpu().numpy()
        for c in check:
            err, want, wused = refs[c].process(x[c, i * m:(i + 1) * m], R441, cap_of(R441, m))
            assert err == 0 and (used, gen) == (wused, len(want))
            assert np.array_equal(bits(a[c]), bits(want)), (c, i)
    assert plan.enqueue_counts() == (0, nmsg)


@pytest.mark.parametrize("nch", [3, 70])
@pytest.mark.parametrize("ratio,conv,queued", [(0.02, 1, True), (R441, 1, False), (R441, 4, False), (0.5, 4, False)])
def test_packed_rows_write_nothing_behind_them(gpu, redio, oracle, ratio, conv, queued, nch):
    segs = [5000, 3001, 4000]
    cuts = cuts_of(segs)
    x = np.stack([oracle.synth_f32(800 + c, 0, cuts[-1]) for c in range(nch)])
    d = gpu.from_numpy(x).cuda()
    plan, twin = redio.Src(nch, conv), redio.Src(nch, conv)
    for i, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        cap = cap_of(ratio, hi - lo) + 5          # capacity above the count: packed rows are closer together than the capacity
        buf = gpu.empty(nch * cap + 64, dtype=gpu.int32, device="cuda")
        buf.fill_(int(CANARY.view(np.int32)))
        q0, s0 = plan.enqueue_counts()
        out, used, gen = plan.enqueue(d[:, lo:hi], ratio, out=buf.view(gpu.float32)[: nch * cap], output_frames=cap, packed=True)
        q1, s1 = plan.enqueue_counts()
        want, wused = twin.process(d[:, lo:hi].contiguous(), ratio, output_frames=cap)
        gpu.cuda.synchronize()
        assert (q1 - q0, s1 - s0) == ((1, 0) if queued and i > 0 else (0, 1))
        assert used == wused and want.shape == (nch, gen) and gen > 0
        h = buf.cpu().numpy().view(np.uint32)
        assert np.array_equal(h[: nch * gen].reshape(nch, gen), bits(want.cpu().numpy()))
        assert np.all(h[nch * gen:] == CANARY), "a write behind the packed rows"
        assert out.shape == (nch, gen) and out.data_ptr() == buf.data_ptr()


def test_mixing_enqueue_process_reset(gpu, redio, oracle):
    # the steps of test_single_launch_then_flush_and_ratio_change: a uniform message, a varying-ratio one, end_of_input; then reset
    n = 90000
    x = oracle.synth_f32(77, 0, n)
    d = gpu.from_numpy(x[None, :]).cuda()
    plan, ref = redio.Src(1, 1), oracle.Resampler(1)

    def step(lo, hi, r, eoi, how):
        cap = cap_of(r, hi - lo) + 400
        if how == "enqueue":
            got, used, gen = plan.enqueue(d[:, lo:hi], r, output_frames=cap)
        else:
            got, used = plan.process(d[:, lo:hi].contiguous(), r, output_frames=cap, end_of_input=bool(eoi))
        err, want, wused = ref.process(x[lo:hi], r, cap, bool(eoi))
        assert err == 0 and used == wused and got.shape[1] == len(want), (lo, hi, r, how)
        assert np.array_equal(bits(got.cpu().numpy()[0]), bits(want)), (lo, hi, r, how)

    step(0, 40000, 0.05, 0, "enqueue")
    step(40000, 70000, 0.07, 0, "enqueue")       # the ratio glides inside the call: the synchronising path
    step(70000, 90000, 0.07, 1, "process")
    assert plan.enqueue_counts() == (0, 2)
    plan.reset()
    ref = oracle.Resampler(1)
    step(0, 30000, 0.05, 0, "enqueue")           # tables of this increment are still there: queued
    step(30000, 60000, 0.05, 0, "enqueue")
    assert plan.enqueue_counts() == (2, 2)
    plan.reset()                                  # reset while queued calls may be in flight
    ref = oracle.Resampler(1)
    step(0, 20000, 0.05, 0, "process")
    step(20000, 40000, 0.05, 0, "enqueue")


def test_fast_mode_through_enqueue(gpu, redio, oracle):
    nch, n, ratio = 4, 100000, 0.02
    x = np.stack([oracle.synth_f32(500 + c, 0, n) for c in range(nch)])
    d = gpu.from_numpy(x).cuda()
    exact, fast, twin = redio.Src(nch, 1), redio.Src(nch, 1, mode=redio.Src.FAST), redio.Src(nch, 1, mode=redio.Src.FAST)
    bound = _fast_bound(oracle, ratio, np.abs(x).max())
    for lo, hi in ((0, 40000), (40000, 40003), (40003, n)):
        a, ua, ga = exact.enqueue(d[:, lo:hi], ratio)
        b, ub, gb = fast.enqueue(d[:, lo:hi], ratio)
        t, ut = twin.process(d[:, lo:hi].contiguous(), ratio)
        gpu.cuda.synchronize()
        assert (ua, ga) == (ub, gb) and ut == ub and t.shape == b.shape
        if ga:
            assert (a - b).abs().max().item() <= bound
        assert np.array_equal(bits(b.cpu().numpy()), bits(t.cpu().numpy()))
    assert fast.enqueue_counts() == (2, 1)


def test_not_capturable_and_state_untouched(gpu, redio, oracle):
    nch, m, ratio = 3, 5000, 0.02
    x = np.stack([oracle.synth_f32(40 + c, 0, 3 * m) for c in range(nch)])
    d = gpu.from_numpy(x).cuda()
    plan = redio.Src(nch, 1)
    refs = [oracle.Resampler(1) for _ in range(nch)]
    out = gpu.empty((nch, cap_of(ratio, m)), dtype=gpu.float32, device="cuda")
    rows = gpu.zeros((64, 4), dtype=gpu.complex64, device="cuda")
    planes = gpu.empty((8, 64), dtype=gpu.float32, device="cuda")

    def checked(i):
        o, used, gen = plan.enqueue(d[:, i * m:(i + 1) * m], ratio, out=out)
        a = o.cpu().numpy()
        for c in range(nch):
            err, want, wused = refs[c].process(x[c, i * m:(i + 1) * m], ratio, cap_of(ratio, m))
            assert err == 0 and (used, gen) == (wused, len(want)) and np.array_equal(bits(a[c]), bits(want)), (i, c)

    checked(0)
    checked(1)
    before = plan.enqueue_counts()
    g = redio.Graph()
    used, gen = C.c_long(5), C.c_long(5)
    with g:
        redio.rows_to_planes(rows, out=planes)    # something capturable, so that the graph is not empty
        part = d[:, 2 * m:3 * m]
        rc = redio.lib().redio_src_enqueue(plan._h, C.c_void_p(part.data_ptr()), m, part.stride(0), C.c_void_p(out.data_ptr()), out.shape[1],
                                           out.stride(0), ratio, C.byref(used), C.byref(gen), redio.current_stream())
    assert rc == -3 and (used.value, gen.value) == (0, 0)
    assert plan.enqueue_counts() == before
    checked(2)                                    # the stream continues where it was


def test_c3_shape_256_channels_two_messages(gpu, redio, oracle):
    """BASELINE.json configs[2] at its channel count through the queued call: 256 mono streams x 2^14 frames in two unequal messages,
    the channels test_c3_256_channels_two_messages checks, bit for bit against the oracle."""
    nch, n, ratio = 256, 1 << 14, 0.02
    x = np.stack([oracle.synth_f32(0x5EED0003 + c, 0, n) for c in range(nch)])
    d = gpu.from_numpy(x).cuda()
    plan = redio.Src(nch, 1)
    check = (0, 1, 31, 63, 64, 100, 127, 128, 191, 192, 200, 254, 255)
    refs = {c: oracle.Resampler(1) for c in check}
    cuts = [0, 9377, n]
    got = [plan.enqueue(d[:, lo:hi], ratio) for lo, hi in zip(cuts[:-1], cuts[1:])]
    gpu.cuda.synchronize()
    for (out, used, gen), lo, hi in zip(got, cuts[:-1], cuts[1:]):
        a = out.cpu().numpy()
        assert used == hi - lo and a.shape == (nch, gen)
        for c in check:
            err, want, wused = refs[c].process(x[c, lo:hi], ratio, cap_of(ratio, hi - lo))
            assert err == 0 and wused == used and np.array_equal(bits(a[c]), bits(want)), (c, lo, hi)
    assert plan.enqueue_counts() == (1, 1)
