"""The stub transport of the exchange tests (tests/stub/fake_rccl.cpp) and the seam it enters through (REDIO_RCCL_LIB, comm.hip).
No device: the stub runs in its host mode, and libredio.so resolves its transport before it touches HIP.  Every case is a fresh
child process (tests/fake_rccl_checks.py), because a transport is loaded once per process; the variable is set only in a child's env."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "_build", "libfake_rccl.so")


@pytest.fixture(scope="module")
def stub():
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "stub"), "-s"])
    assert os.path.exists(STUB)
    return STUB


def child(args, **env):
    e = dict(os.environ)
    e.pop("REDIO_RCCL_LIB", None)
    e.update(env)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "fake_rccl_checks.py")] + [str(a) for a in args], capture_output=True, text=True,
                         env=e, timeout=120, cwd=ROOT)
    assert out.returncode == 0 and '"ok": true' in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


@pytest.mark.parametrize("form", ["one", "threads"])
@pytest.mark.parametrize("n", [2, 3, 8])
def test_stub_all_to_all_delivers_every_byte(stub, n, form):
    """An all-to-all with a different count per pair and a third of the pairs absent, from one thread in one group (the
    redio_pfb_exchange_all shape) and from one thread per rank over ncclCommInitRank (the redio_pfb_exchange shape)."""
    child(["all_to_all", n, form], FAKE_RCCL_HOST="1", FAKE_RCCL_TIMEOUT_MS="20000")


@pytest.mark.parametrize("rule", ["count", "type", "peer", "no_group", "end_without_start", "timeout", "destroyed", "join"])
def test_stub_refuses(stub, rule):
    """One rule per case: the stated error comes back and the counters read as the rule says."""
    child(["refuse", rule], FAKE_RCCL_HOST="1", FAKE_RCCL_TIMEOUT_MS="1000" if rule == "timeout" else "20000")


def test_seam_loads_the_named_transport(stub, redio):
    """REDIO_RCCL_LIB names the stub: redio_comm_unique_id returns the stub's id, and the stub's names stay out of the global namespace."""
    child(["seam", "ok"], REDIO_RCCL_LIB=stub, FAKE_RCCL_HOST="1")


def test_seam_missing_library_is_an_error_that_names_the_path(stub, redio, tmp_path):
    child(["seam", "missing"], REDIO_RCCL_LIB=str(tmp_path / "no_such_transport.so"))


def test_seam_library_without_the_entry_points_is_an_error(stub, redio):
    """A loadable library that is no transport (the product's own kissfft shim): refused by name, and the real RCCL is not tried."""
    import libredio_amd as R
    child(["seam", "no_symbol"], REDIO_RCCL_LIB=R.LIBKISSFFT)
