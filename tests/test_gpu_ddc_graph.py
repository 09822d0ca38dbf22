"""The tuner under stream capture (an enqueue neither allocates nor synchronises), and dev::tuner, dev::tuner_u8 and their _stream forms
(include/kpn_dev.hpp) in a device-resident graph through tests/cpp_ddc: source -> block -> sink, eight messages, against the bare calls
(in the driver, on the device) and against the oracle (here).  The driver runs in a child process."""
import os
import subprocess

import numpy as np
import pytest

import ddc_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EEDDDC3


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("K,D", [(127, 5), (31, 2), (5, 9),
                                 (15008, 1)])  # the chunked route's longest tile, 150 KiB: its first enqueue ever is the captured one
def test_capture_and_replay_and_no_allocation(gpu, redio, oracle, K, D, u8):
    L, first = 4099, 2 ** 32 + 5
    n = 2 * ref.tile_out(K, D) * D + K + 5
    taps, w = oracle.synth_f32(3, K, K), oracle.synth_iq(7, L, L)
    raw = np.random.default_rng(SEED).integers(0, 256, 2 * n, dtype=np.uint8)
    xh = oracle.data_to_samples(raw) if u8 else oracle.synth_iq(SEED, 1, n)
    want = ref.ddc(xh, w, taps, D, True, first)
    d = gpu.from_numpy(raw if u8 else xh).cuda()
    out = gpu.zeros(len(want), dtype=gpu.complex64, device="cuda")
    plan = redio.Ddc(w, taps, D, fused=True)
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
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_ddc"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_ddc_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


def lens(K, D):
    return [K + 40 * D + (101 if i % 2 == 0 else -37) for i in range(8)]


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    made = {}
    for K, D, L in [(127, 5, 24), (31, 2, 4099)]:
        d = tmp_path_factory.mktemp("ddc")
        taps, w = oracle.synth_f32(3, K, K), (ref.osc_table_ref(-5, 24) if L == 24 else oracle.synth_iq(7, L, L))
        tp, wp = str(d / "taps.f32"), str(d / "osc.c32")
        taps.tofile(tp); w.tofile(wp)
        ls = lens(K, D)
        n = sum(ls)
        raw = np.random.default_rng(SEED + K).integers(0, 256, 2 * n, dtype=np.uint8)
        for kind, x in (("cf32", oracle.synth_iq(SEED, K, n)), ("u8", oracle.data_to_samples(raw))):
            path = str(d / f"input.{kind}")
            (raw if kind == "u8" else x).tofile(path)
            stream = ref.ddc(x, w, taps, D, True, 0)                       # history and phase carried
            starts = np.cumsum([0] + ls[:-1])
            blocks = np.concatenate([ref.ddc(x[s: s + m], w, taps, D, True, 0) for s, m in zip(starts, ls)])  # the phase restarts per message
            made[(K, D, kind)] = (wp, tp, path, stream, blocks)
    return made


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("kind", ["cf32", "u8"])
@pytest.mark.parametrize("mode", ["stream", "blocks"])
@pytest.mark.parametrize("K,D", [(127, 5), (31, 2)])
def test_tuner_blocks(gpu, redio, cases, tmp_path, K, D, mode, kind, depth):
    wp, tp, path, stream, blocks = cases[(K, D, kind)]
    want = stream if mode == "stream" else blocks
    assert len(stream) > len(blocks) and not np.array_equal(bits(stream[: len(blocks)]), bits(blocks))  # the two semantics differ
    out = tmp_path / f"{mode}{depth}.bin"
    line = driver(mode, str(depth), kind, str(D), "1", wp, tp, path, str(out)).split()
    assert line[:7] == [mode, str(depth), "msgs", "8", "samples", str(len(want)), "bare_equal"] and line[7] == "1", line
    got = np.fromfile(out, np.complex64)
    assert np.array_equal(bits(got), bits(want))
