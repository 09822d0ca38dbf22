"""The coalescing loop of include/kpn_dev.hpp (detail::run_block_list) on the CPU: host memory through the dev::DeviceApi stand-ins
(tests/cpp_list/kpn_list_tests.cpp `list_plumbing`): order, boundaries and contents of the messages, batches that really form, the
ring's bound, a hang-up with a batch open, and no deadlock behind a producer ring of one buffer."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "kpn_list_tests")


def test_list_plumbing_cpu(redio, tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp_list"), "-s"])
    out = subprocess.run([EXE, "list_plumbing"], capture_output=True, text=True, timeout=600, env=dict(os.environ, TMPDIR=str(tmp_path)))
    assert out.returncode == 0 and "list_plumbing ok" in out.stdout, out.stderr
