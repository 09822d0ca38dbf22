"""dev::power_spectrum_real_stream and dev::power_spectrum_real (include/kpn_dev.hpp) in a device-resident graph, through
tests/cpp_pspec_real: source -> block -> sink through rings of 1 and 2 buffers, on the fused size (2048, K = 17, step 1024, windowed)
and a generic one (64, K = 33); the sink's rows bit for bit against the bare calls' (tests/pspec_real_ref.py, which
tests/test_gpu_pspec_real.py ties to them), and no device allocation after the first message."""
import os
import subprocess

import numpy as np
import pytest

import pspec_real_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0B5D
SHAPES = [(2048, 17, 1024, True), (64, 33, 64, False)]


def stream_lens(W, H):
    return [W + 2 * H] + [2 * H + 100 if i % 2 else 2 * H - 100 for i in range(10)]


def block_lens(W, H):
    return [W + (rows - 1) * H for rows in (3, 1, 2)] * 4


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_pspec_real"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_pspec_real_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """per shape: the window file's path (or "none"), the stream's rows and the per-message rows, computed once"""
    made = {}
    for N, K, step, windowed in SHAPES:
        W, H = ref.shape(N, K, step)
        w, path = None, "none"
        if windowed:
            w = oracle.lpf_corrected(N, 0.1)
            path = str(tmp_path_factory.mktemp("pspec_real") / "window.f32")
            w.tofile(path)
        sl, bl = stream_lens(W, H), block_lens(W, H)
        x = oracle.synth_f32(SEED, 0, max(sum(sl), sum(bl)))
        stream = ref.power_spectrum(x[: sum(sl)], N, K, step, w)
        starts = np.cumsum([0] + bl[:-1])
        blocks = np.concatenate([ref.power_spectrum(x[s: s + n], N, K, step, w) for s, n in zip(starts, bl)])
        made[(N, K, step)] = (path, stream, blocks)
    return made


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("N,K,step,windowed", SHAPES)
def test_stream_graph(gpu, redio, cases, tmp_path, N, K, step, windowed, depth):
    path, want, _ = cases[(N, K, step)]
    out = tmp_path / f"stream{depth}.bin"
    line = driver("stream", str(depth), str(N), str(K), str(step), path, str(out)).split()
    assert want.shape == (3 + 5 * (1 + 3), N // 2 + 1)  # every message completes at least one row
    assert line == ["stream", str(depth), "msgs", "11", "words", str(want.size), "mallocs_after_first", "0"]
    got = np.fromfile(out, np.float32)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("N,K,step,windowed", SHAPES)
def test_whole_row_messages_graph(gpu, redio, cases, tmp_path, N, K, step, windowed, depth):
    path, _, want = cases[(N, K, step)]
    out = tmp_path / f"blocks{depth}.bin"
    line = driver("blocks", str(depth), str(N), str(K), str(step), path, str(out)).split()
    assert want.shape == (4 * (3 + 1 + 2), N // 2 + 1)
    assert line == ["blocks", str(depth), "msgs", "12", "words", str(want.size), "mallocs_after_first", "0"]
    got = np.fromfile(out, np.float32)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))
