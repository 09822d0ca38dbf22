"""dev::oversampled_channelizer and dev::oversampled_channelizer_stream (include/kpn_dev.hpp) with one_kernel = true in a
device-resident graph, through tests/cpp_pfb_os_p2: source -> block -> sink on two route-2 shapes; the sink's samples bit for bit
against the Python plan with one_kernel=True, the oracle restatement (tests/pfb_os_ref.py) and the bare calls on a flagged plan, and no
device allocation after the first message."""
import os
import subprocess

import numpy as np
import pytest

import pfb_os_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0B55
SHAPES = [(128, 8), (512, 4)]


def lens(M, P):
    """the driver's messages (tests/cpp_pfb_os_p2): the first is P + 1 rows of M longer, so no later message of the stream yields more"""
    return [(P + 40 + (0 if i else P + 1)) * M + (101 if i % 2 == 0 else -37) for i in range(8)]


def driver(*args):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_pfb_os_p2"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_pfb_os_p2_tests"), *args], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return out.stdout


@pytest.fixture(scope="module")
def cases(gpu, redio, oracle, tmp_path_factory):
    """per shape: the files' paths and the two expected outputs from the Python plan, held to the restatement; computed once"""
    made = {}
    for M, P in SHAPES:
        H = M // 2
        d = tmp_path_factory.mktemp("pfb_os_p2")
        h = oracle.synth_f32(9, 0, M * P)
        ll = lens(M, P)
        x = oracle.synth_iq(SEED, M, sum(ll))
        proto, path = str(d / "proto.f32"), str(d / "input.cf32")
        h.tofile(proto)
        x.tofile(path)
        plan = redio.OversampledChannelizer(h, M, P, H, fused=True, one_kernel=True)
        assert plan.route == 2
        xd = gpu.from_numpy(x).cuda()
        starts = np.cumsum([0] + ll[:-1])
        stream = plan(xd, first_row=0).cpu().numpy().reshape(-1)
        blocks = np.concatenate([plan(xd[s: s + m], first_row=0).cpu().numpy().reshape(-1) for s, m in zip(starts, ll)])
        assert np.array_equal(stream.view(np.uint32), ref.channelize(x, h, M, P, H, 0, True).reshape(-1).view(np.uint32))
        made[(M, P)] = (proto, path, {"stream": stream, "blocks": blocks})
    return made


@pytest.mark.parametrize("mode,depth", [("stream", 1), ("stream", 2), ("blocks", 2)])
@pytest.mark.parametrize("M,P", SHAPES)
def test_blocks_and_stream_blocks(cases, tmp_path, M, P, mode, depth):
    proto, path, wants = cases[(M, P)]
    want = wants[mode]
    out = tmp_path / f"{mode}{depth}.bin"
    line = driver(mode, str(depth), str(M), str(P), str(M // 2), "1", proto, path, str(out)).split()
    assert line == [mode, str(depth), "route", "2", "msgs", "8", "samples", str(want.size), "bare_equal", "1", "mallocs_after_first", "0"]
    got = np.fromfile(out, np.complex64)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
