"""The rational resampler under stream capture (an enqueue neither allocates nor synchronises) on both routes, and dev::upfirdn and
dev::upfirdn_stream (include/kpn_dev.hpp) in a device-resident graph through tests/cpp_upfirdn: source -> block -> sink, eight messages,
against the bare calls (in the driver, on the device) and against the reference (here).  The driver runs in a child process."""
import os
import subprocess

import numpy as np
import pytest

import upfirdn_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDF1D3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("U,D,K,route", [(3, 2, 64, 1), (16, 1, 255, 1), (3, 16, 33, 2),
                                         (2, 1, 25396, 1)])  # a tile above 48 KiB as f32 and as cf32: its first enqueue ever is the captured one
def test_capture_and_replay_and_no_allocation(gpu, redio, oracle, U, D, K, route, cplx):
    n = ref.n_for(2 * ref.tile_out(K, U, D) + 5, K, U, D)
    taps = oracle.synth_f32(3, K, K)
    xh = oracle.synth_iq(SEED, 1, n) if cplx else oracle.synth_f32(SEED, 1, n)
    want = ref.upfirdn(xh, taps, U, D, True)
    d = gpu.from_numpy(xh).cuda()
    out = gpu.zeros(len(want), dtype=d.dtype, device="cuda")
    plan = redio.Upfirdn(taps, U, D, complex_input=cplx, fused=True)
    assert plan.route == route
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        plan(d, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    for _ in range(100):
        plan(d, out=out)
    gpu.cuda.synchronize()
    assert redio.lib().redio_malloc_count() == count  # neither the capture nor 100 enqueues allocated


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_upfirdn"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_upfirdn_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def lens(K, U, D):
    return [ref.window(K, U, D) + 40 * ref.periods(U, D)[1] + (101 if i % 2 == 0 else -37) for i in range(8)]


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    made = {}
    for U, D, K in [(3, 2, 64), (17, 1, 40)]:
        d = tmp_path_factory.mktemp("upfirdn")
        taps = oracle.synth_f32(3, K, K)
        tp = str(d / "taps.f32")
        taps.tofile(tp)
        ls = lens(K, U, D)
        n = sum(ls)
        Up, Dp = ref.periods(U, D)
        for kind, x in (("f32", oracle.synth_f32(SEED, K, n)), ("cf32", oracle.synth_iq(SEED, K, n))):
            path = str(d / f"input.{kind}")
            x.tofile(path)
            stream = ref.upfirdn(x, taps, U, D, True)[: Up * ((n - ref.window(K, U, D)) // Dp + 1)]  # history carried: whole periods
            starts = np.cumsum([0] + ls[:-1])
            blocks = np.concatenate([ref.upfirdn(x[s: s + m], taps, U, D, True) for s, m in zip(starts, ls)])  # every message on its own
            made[(U, D, K, kind)] = (tp, path, stream, blocks)
    return made


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("kind", ["f32", "cf32"])
@pytest.mark.parametrize("mode", ["stream", "blocks"])
@pytest.mark.parametrize("U,D,K", [(3, 2, 64), (17, 1, 40)])
def test_resampler_blocks(gpu, redio, cases, tmp_path, U, D, K, mode, kind, depth):
    tp, path, stream, blocks = cases[(U, D, K, kind)]
    want = stream if mode == "stream" else blocks
    assert len(stream) > len(blocks) and not np.array_equal(bits(stream[: len(blocks)]), bits(blocks))  # the two semantics differ
    out = tmp_path / f"{mode}{depth}.bin"
    line = driver(mode, str(depth), kind, str(U), str(D), "1", tp, path, str(out)).split()
    assert line[:7] == [mode, str(depth), "msgs", "8", "samples", str(len(want)), "bare_equal"] and line[7] == "1", line
    got = np.fromfile(out, np.float32 if kind == "f32" else np.complex64)
    assert np.array_equal(bits(got), bits(want))
