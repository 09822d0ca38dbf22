"""dev::resample_channels, dev::channel_planes and dev::plane_rows (include/kpn_dev.hpp) in device-resident graphs, through
tests/cpp_src: the graph's checksum and per-message lengths against the same calls made bare, no device allocation after warm-up, and
one synchronising resampler call per graph (the first, which builds the tables)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_channels_graph(gpu, redio):
    lines = [l.split() for l in subprocess_lines("src_gpu")]
    assert [(l[1], l[2]) for l in lines] == [("shared", "4"), ("shared", "1"), ("per_block", "4"), ("per_block", "1")]
    for l in lines:
        f = dict(zip(l[3::1], l[4::1]))
        assert l[3] == "graph" and l[6] == "bare"
        assert l[4] == l[7] and l[5] == l[8] == "40", l          # checksum and message count
        assert f["lens_equal"] == "1", l
        assert f["mallocs_after_2"] == "0", l
        assert f["synchronised"] == "1" and f["queued"] == "39", l


def test_channelizer_planes_resampler_rows_graph(gpu, redio):
    lines = [l.split() for l in subprocess_lines("c4c3")]
    assert len(lines) == 1
    l = lines[0]
    f = dict(zip(l[1::1], l[2::1]))
    assert l[1] == "graph" and l[4] == "bare"
    assert l[2] == l[5] and l[3] == l[6] == "12" and int(l[2]) != 0, l
    assert f["lens_equal"] == "1" and f["synchronised"] == "1" and f["queued"] == "11", l


def subprocess_lines(mode):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_src"), "-s"])
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_src_tests"), mode], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    return [l for l in out.stdout.splitlines() if l.startswith(mode + " ")]
