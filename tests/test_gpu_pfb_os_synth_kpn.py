"""dev::oversampled_synthesizer and dev::oversampled_synthesizer_stream (include/kpn_dev.hpp) in a device-resident graph, through
tests/cpp_pfb_os_synth: source -> block -> sink through rings of 1 and 2 buffers on the wave kernel's shape (64 x 16, hop 32) and a
two-pass one (128 x 4, hop 48); the sink's samples bit for bit against the restatement (tests/pfb_os_synth_ref.py) and the bare calls,
and no device allocation after the first message.  The plan has no list entry point, so the blocks take one message per launch."""
import os
import subprocess

import numpy as np
import pytest

import pfb_os_synth_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0537
SHAPES = [(64, 16, 32), (128, 4, 48)]


def lens(M, P, H):
    """the driver's messages; the first is L + 1 rows of M longer, so no later message of the stream yields more than it"""
    L = ref.nrows_per_hop(M, P, H)
    return [(L + 40 + (0 if i else L + 1)) * M + (101 if i % 2 == 0 else -37) for i in range(8)]


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_pfb_os_synth"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_pfb_os_synth_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def cases(oracle, tmp_path_factory):
    """per shape: the prototype's and the input file's paths and the two expected outputs, computed once"""
    made = {}
    for M, P, H in SHAPES:
        d = tmp_path_factory.mktemp("pfb_os_synth")
        h = oracle.synth_f32(9, 0, M * P)
        ll = lens(M, P, H)
        X = oracle.synth_iq(SEED, M, sum(ll))
        proto, path = str(d / "proto.f32"), str(d / "input.cf32")
        h.tofile(proto)
        X.tofile(path)
        starts = np.cumsum([0] + ll[:-1])
        made[(M, P, H)] = (proto, path, {
            "stream": ref.synth(X, h, M, P, H, 0, True),
            "blocks": np.concatenate([ref.synth(X[s: s + m], h, M, P, H, 0, True) for s, m in zip(starts, ll)]),
        })
    return made


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("mode", ["stream", "blocks"])
@pytest.mark.parametrize("M,P,H", SHAPES)
def test_blocks_and_stream_blocks(gpu, redio, cases, tmp_path, M, P, H, mode, depth):
    proto, path, wants = cases[(M, P, H)]
    want = wants[mode]
    out = tmp_path / f"{mode}{depth}.bin"
    line = driver(mode, str(depth), str(M), str(P), str(H), "1", proto, path, str(out)).split()
    assert line == [mode, str(depth), "msgs", "8", "samples", str(want.size), "bare_equal", "1", "mallocs_after_first", "0"]
    got = np.fromfile(out, np.complex64)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
