"""The tuned resampler under stream capture (an enqueue neither allocates nor synchronises), and dev::tuned_resampler,
dev::tuned_resampler_u8 and their _stream forms (include/kpn_dev.hpp) in a device-resident graph through tests/cpp_ddc_upfirdn:
source -> block -> sink, eight messages, against the bare calls (in the driver, on the device) and against the reference (here).  The
driver runs in a child process."""
import os
import subprocess

import numpy as np
import pytest

import ddc_ref
import ddc_upfirdn_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED17D3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("U,D,K", [(3, 2, 64), (4, 5, 100), (2, 7, 9),
                                   (2, 1, 36863)])  # route 1's longest tile at 2/1, above 48 KiB: its first enqueue ever is the captured one
def test_capture_and_replay_and_no_allocation(gpu, redio, oracle, U, D, K, u8):
    L, first = 4099, 2 ** 32 + 5
    n = ref.n_for(2 * ref.tile_out(K, U, D) + 5, K, U, D)
    taps, w = oracle.synth_f32(3, K, K), oracle.synth_iq(7, L, L)
    raw = np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8)
    xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, 1, n)
    want = ref.ddc_upfirdn(xh, w, taps, U, D, True, first)
    d = gpu.from_numpy(raw if u8 else xh).cuda()
    out = gpu.zeros(len(want), dtype=gpu.complex64, device="cuda")
    plan = redio.DdcUpfirdn(w, taps, U, D, fused=True)
    run = plan.from_bytes if u8 else plan
    count = redio.lib().redio_malloc_count()
    g = redio.Graph()
    with g:
        run(d, first=first, out=out)
    for _ in range(2):
        out.zero_()
        g.launch()
        gpu.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    for i in range(100):
        run(d, first=first + i, out=out)
    gpu.cuda.synchronize()
    assert redio.lib().redio_malloc_count() == count  # neither the capture nor 100 enqueues allocated


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_ddc_upfirdn"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_ddc_upfirdn_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def lens(K, D):
    return [K + 40 * D + (101 if i % 2 == 0 else -37) for i in range(8)]


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    made = {}
    for U, D, K, L in [(3, 2, 64, 24), (2, 7, 9, 4099)]:
        d = tmp_path_factory.mktemp("ddc_upfirdn")
        taps, w = oracle.synth_f32(3, K, K), (ddc_ref.osc_table_ref(-5, 24) if L == 24 else oracle.synth_iq(7, L, L))
        tp, wp = str(d / "taps.f32"), str(d / "osc.c32")
        taps.tofile(tp); w.tofile(wp)
        ls = lens(K, D)
        n = sum(ls)
        Up, Dp = ref.periods(U, D)
        raw = np.random.default_rng(SEED + K).integers(0, 256, 2 * n, dtype=np.uint8)
        for kind, x in (("cf32", oracle.synth_iq(SEED, K, n)), ("u8", oracle.data_to_samples(raw))):
            path = str(d / f"input.{kind}")
            (raw if kind == "u8" else x).tofile(path)
            stream = ref.ddc_upfirdn(x, w, taps, U, D, True, 0)[: Up * ((n - ref.window(K, U, D)) // Dp + 1)]  # history and phase carried: whole periods
            starts = np.cumsum([0] + ls[:-1])
            blocks = np.concatenate([ref.ddc_upfirdn(x[s: s + m], w, taps, U, D, True, 0) for s, m in zip(starts, ls)])  # phase and table restart per message
            made[(U, D, K, kind)] = (wp, tp, path, stream, blocks)
    return made


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("kind", ["cf32", "u8"])
@pytest.mark.parametrize("mode", ["stream", "blocks"])
@pytest.mark.parametrize("U,D,K", [(3, 2, 64), (2, 7, 9)])
def test_tuned_resampler_blocks(gpu, redio, cases, tmp_path, U, D, K, mode, kind, depth):
    wp, tp, path, stream, blocks = cases[(U, D, K, kind)]
    want = stream if mode == "stream" else blocks
    assert len(stream) > len(blocks) and not np.array_equal(bits(stream[: len(blocks)]), bits(blocks))  # the two semantics differ
    out = tmp_path / f"{mode}{depth}.bin"
    line = driver(mode, str(depth), kind, str(U), str(D), "1", wp, tp, path, str(out)).split()
    assert line[:7] == [mode, str(depth), "msgs", "8", "samples", str(len(want)), "bare_equal"] and line[7] == "1", line
    got = np.fromfile(out, np.complex64)
    assert np.array_equal(bits(got), bits(want))
