"""The tuner as a stream (redio_ddc_stream_*): carried history AND carried phase -- any segmentation of the input gives the bits of one
redio_ddc_enqueue on the whole stream with first_index 0."""
import ctypes as C

import numpy as np
import pytest

import ddc_ref as ref

pytestmark = pytest.mark.gpu

SEED = 0x5EEDDDC2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def cuts(rng, n, style):
    """the cut styles of test_gpu_streams.py"""
    if style == "one":
        return [n]
    lo, hi = {"tiny": (0, 40), "small": (1, 900)}.get(style, (0, 0))
    out, left = [], n
    while left:
        if style == "odd":
            k = 2 * int(rng.integers(500, 40000)) + 1
        elif style == "mixed":
            k = int(rng.choice([1, 7, 126, 127, 128, 1000, 5119, 5120, 5121, 5246, 20000, 65536, 100001]))
        else:
            k = int(rng.integers(lo, hi))
        k = min(left, k)
        out.append(k); left -= k
    return out


@pytest.fixture(scope="module")
def streams(oracle):
    """per (taps, decimation, period, u8, length): the input and the one-shot outputs with first = 0 of both folds, computed once"""
    made = {}

    def get(K, D, L, u8, n):
        key = (K, D, L, u8, n)
        if key not in made:
            taps = oracle.synth_f32(5, K, K)
            w = ref.osc_table_ref(-5, 24) if L == 24 else oracle.synth_iq(7, L, L)
            raw = np.random.default_rng(SEED + K + L).integers(0, 256, 2 * n, dtype=np.uint8)
            xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, L, n)
            m = ref.mixed(xh, w, 0)
            want = {f: oracle.fir(m, taps, D, f) for f in (False, True)}
            for a in want.values():
                a.setflags(write=False)
            made[key] = (taps, w, raw if u8 else xh, want)
        return made[key]
    return get


@pytest.mark.parametrize("style", ["one", "tiny", "small", "odd", "mixed"])
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("L", [24, 4099])
@pytest.mark.parametrize("K,D,fused", [(127, 5, True), (31, 2, False), (5, 9, True),
                                       (15008, 1, False)])  # the last tap count of the chunked route: 15007 samples carried, a tile of 150 KiB
def test_any_segmentation_equals_the_one_shot_call(gpu, redio, streams, K, D, fused, L, u8, style):
    rng = np.random.default_rng(K * 131 + D + L)
    n = 3 * L + 2000 if style == "tiny" else (3 * L + 40000 if style == "small" else 3 * L + 150000)  # longer than 3 L: the phase wraps across seams
    if K > 1000:  # the oracle's cost is outputs x taps: the filter's length and 2000 or 20000 outputs behind it
        n = 3 * L + K + (2000 if style == "tiny" else 20000)
    taps, w, src, want = streams(K, D, L, u8, n)
    want = want[fused]
    x = gpu.from_numpy(src).cuda()
    E = 2 if u8 else 1
    plan = redio.Ddc(w, taps, D, fused=fused)
    st = redio.Stream(plan, u8=u8)
    assert st.index == 0
    outs, pos = [], 0
    for k in cuts(rng, n, style):
        expect = st.nout(k)
        y = st(x[E * pos: E * (pos + k)])
        assert y.numel() == expect
        outs.append(y.clone())
        pos += k
        assert st.index == pos  # redio_ddc_stream_index: the next new sample
    got = gpu.cat(outs).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (K, D, L, style)
    if K >= D:
        assert st.pending == max(n - len(want) * D, 0) and st.pending < K
    # reset restarts the phase with the history
    st.reset()
    assert st.index == 0 and st.pending == 0
    half = n // 2 + 1
    again = gpu.cat([st(x[: E * half]).clone(), st(x[E * half:]).clone()]).cpu().numpy()
    assert np.array_equal(bits(again), bits(want)) and st.index == n
    one = (plan.from_bytes if u8 else plan)(x, first=0).cpu().numpy()
    assert np.array_equal(bits(one), bits(want))


def test_concurrent_entry_is_refused_and_a_failed_call_keeps_its_state(gpu, redio, oracle):
    import threading
    L = redio.lib()
    K = 33
    plan = redio.Ddc(oracle.synth_iq(7, 24, 24), oracle.synth_f32(5, 0, K), 1)
    st = redio.Stream(plan)
    x = gpu.from_numpy(oracle.synth_iq(11, 0, 4096)).cuda()
    y = [gpu.empty(4096, dtype=gpu.complex64, device="cuda") for _ in range(2)]
    gpu.cuda.synchronize()
    stream = redio.current_stream()
    ok_samples, ok_out, refused = [0, 0], [0, 0], [0, 0]
    go = threading.Barrier(2)

    def work(t):
        go.wait()
        for _ in range(2000):
            got = C.c_size_t(0)
            rc = L.redio_ddc_stream_enqueue(st._h, C.c_void_p(x.data_ptr()), 64, C.c_void_p(y[t].data_ptr()), C.byref(got), stream)
            if rc == 0:
                ok_samples[t] += 64; ok_out[t] += got.value
            else:
                assert rc == -1, rc
                refused[t] += 1
    th = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in th: t.start()
    for t in th: t.join()
    gpu.cuda.synchronize()
    total = sum(ok_samples)
    assert total > 0 and sum(ok_out) == total - (K - 1), (ok_samples, ok_out, refused)
    assert st.pending == K - 1 and st.index == total
    # a failed call changes nothing: outputs are due, no output buffer
    got = C.c_size_t(0)
    assert L.redio_ddc_stream_enqueue(st._h, C.c_void_p(x.data_ptr()), 100, None, C.byref(got), stream) == -1
    assert st.pending == K - 1 and st.index == total and st.nout(100) == 100
    # and the stream goes on from where it was: the next call's outputs are the one-shot call's at that stream index
    st.reset()
    a = st(x[:1000]).clone()
    assert L.redio_ddc_stream_enqueue(st._h, C.c_void_p(x.data_ptr()), 100, None, C.byref(got), stream) == -1
    b = st(x[1000:]).clone()
    want = plan(x, first=0)
    assert np.array_equal(bits(gpu.cat([a, b]).cpu().numpy()), bits(want.cpu().numpy()))
