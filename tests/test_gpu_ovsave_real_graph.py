"""dev::overlap_save_real_stream and dev::overlap_save_real (include/kpn_dev.hpp) in a device-resident graph, through
tests/cpp_ovsave_real: source -> block(127 taps, 2048) -> sink over 12 messages, through rings of 1 and 2 buffers; the sink's words bit
for bit against tests/ovsave_real_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import ovsave_real_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N, K = 0x5EED0A5E, 2048, 127
HOP = N - K + 1
STREAM_LENS = [1, 7, 1921, 1922, 2048, 2049, 6149, 333, 4097, 1000, 5001, 12345]
BLOCK_LENS = [N + (nb - 1) * HOP for nb in (1, 2, 5)] * 4


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_ovsave_real"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_ovsave_real_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def taps(oracle, tmp_path_factory):
    t = oracle.lpf_corrected(K, 0.08)
    path = tmp_path_factory.mktemp("ovsr") / "taps.f32"
    t.tofile(path)
    return t, str(path)


@pytest.fixture(scope="module")
def expected(oracle, taps):
    x = oracle.synth_f32(SEED, 0, max(sum(STREAM_LENS), sum(BLOCK_LENS)))
    stream = ref.overlap_save_real(x[: sum(STREAM_LENS)], taps[0], N)
    starts = np.cumsum([0] + BLOCK_LENS[:-1])
    blocks = np.concatenate([ref.overlap_save_real(x[s: s + n], taps[0], N) for s, n in zip(starts, BLOCK_LENS)])
    return stream, blocks


@pytest.mark.parametrize("depth", [1, 2])
def test_stream_graph(gpu, redio, taps, expected, tmp_path, depth):
    path = tmp_path / f"stream{depth}.bin"
    line = driver("stream", str(depth), taps[1], str(path)).split()
    want = expected[0]
    sent, total, msgs = 0, 0, 0  # a message that completes no block sends nothing
    for n in STREAM_LENS:
        total += n
        now = ref.nout(total, K, N)
        msgs += now > sent
        sent = now
    assert len(want) == sent
    assert line == ["stream", str(depth), "msgs", str(msgs), "words", str(len(want))]
    got = np.fromfile(path, np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("depth", [1, 2])
def test_whole_block_messages_graph(gpu, redio, taps, expected, tmp_path, depth):
    path = tmp_path / f"blocks{depth}.bin"
    line = driver("blocks", str(depth), taps[1], str(path)).split()
    want = expected[1]
    assert len(want) == 4 * (1 + 2 + 5) * HOP
    assert line == ["blocks", str(depth), "msgs", "12", "words", str(len(want))]
    got = np.fromfile(path, np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
