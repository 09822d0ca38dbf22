"""dev::fftr and dev::fftri (include/kpn_dev.hpp) in a device-resident graph, through tests/cpp_fftr: source -> fftr(2048) -> fftri(2048) ->
sink over 12 messages of 1, 2 and 5 blocks, through rings of 1 and 2 buffers; the sink's words bit for bit against tests/fftr_ref.py."""
import os
import subprocess

import numpy as np
import pytest

import fftr_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, N, BLOCKS = 0x5EED0F7A, 2048, 4 * (1 + 2 + 5)


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_fftr"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_fftr_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def expected(oracle):
    x = oracle.synth_f32(SEED, 0, BLOCKS * N)
    return fftr_ref.fftri_rows(fftr_ref.fftr_rows(x, N), N).reshape(-1)


@pytest.mark.parametrize("depth", [1, 2])
def test_round_trip_graph(gpu, redio, expected, tmp_path, depth):
    path = tmp_path / f"sink{depth}.bin"
    line = driver("round_trip", str(depth), str(path)).split()
    assert line == ["round_trip", str(depth), "msgs", "12", "words", str(BLOCKS * N)]
    got = np.fromfile(path, np.float32)
    assert np.array_equal(got.view(np.uint32), expected.view(np.uint32))


def test_message_of_2047_samples(gpu, redio):
    assert driver("short_message").strip() == "short_message assert!(din.len() == block_size) (kissfft.rs:24)"
