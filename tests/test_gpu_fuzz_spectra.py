"""A short, seeded run of the second randomised differential tool (tests/fuzz_spectra.py) per family: the real-input transform,
overlap-save on real streams, the power spectrum from cf32 samples, from u8 bytes and from real samples, their streams, and the polyphase
spectrometer (cf32 and bytes; the wave kernel, the workgroup kernel of one_kernel=True and the generic route) and its streams, bit for bit against the restatements on random shapes, steps, windows, split modes, alignments and message cuts.  Each run starts with the tool's
opening round of 24 cases, so its route coverage (tests/test_spectra_fuzz_cpu.py) does not depend on the machine's speed."""
import ast
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11  # tests/test_spectra_fuzz_cpu.py checks the generator's coverage at this seed
FAMILIES = ["fftr", "ovsave_real", "pspec", "pspec_u8", "pspec_real", "streams", "pfb_pspec", "pfb_streams"]


@pytest.mark.parametrize("family", FAMILIES)
def test_randomised_differential_run_of_the_spectrum_plans(gpu, family):
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fuzz_spectra.py"), "4", str(SEED), "--only", family]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:  # reported, not retried
        pytest.fail(f"{family}: no end after {e.timeout} s\n{(e.stdout or b'')[-3000:]}\n{(e.stderr or b'')[-2000:]}")
    tail = out.stdout[-3000:] + out.stderr[-2000:]
    assert out.returncode >= 0, f"{family}: the child died on signal {-out.returncode}\n{tail}"
    assert out.returncode == 0, tail
    assert "failures 0" in out.stdout, tail
    summary = [ln for ln in out.stdout.splitlines() if ln.startswith("runs ")][-1]
    runs = ast.literal_eval(summary[len("runs "): summary.rindex(" failures")])
    print(family, runs)
    assert runs.get(family, 0) >= 24, summary
    if family in ("pfb_pspec", "pfb_streams"):   # the polyphase spectrometer's workgroup kernel ran: the tool's own count of its route-2 cases
        assert runs.get(family + " route 2", 0) >= 1, summary
