"""The channelizer's exchange (libredio_amd/csrc/comm.hip: redio_pfb_exchange, _at, _all) at 2 to 8 ranks on ONE device.

Real RCCL refuses two ranks on one GPU, and no box this project has run on has two, so the exchange had only ever executed with one rank,
where every offset in it is zero.  Here a stub transport (tests/stub/fake_rccl.cpp, named to libredio.so by REDIO_RCCL_LIB) matches the
sends and receives of all ranks and copies device to device in stream order, so the buffer arithmetic, the pairing across ranks and
2^27-float pieces, argument handling and device state run for real; the result must be the oracle's channelizer of the whole stream,
bit for bit.  What this cannot show (RCCL's own ordering, a real transfer's 1 GiB limit, link rates): DESIGN.md 5.11.

Each test is ONE child process (tests/exchange_rank_checks.py) that holds all ranks, under a time limit; the variable is set only in
the child's environment.  The stub turns an unpaired send or receive into an error after FAKE_RCCL_TIMEOUT_MS, never a hang, and every
child ends by asserting that the stub saw no unmatched operation and returned no error."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "_build", "libfake_rccl.so")


@pytest.fixture(scope="module")
def stub(redio):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "stub"), "-s"])
    assert os.path.exists(STUB)
    return STUB


def child(stub, *args):
    env = dict(os.environ)
    env.update(REDIO_RCCL_LIB=stub)
    env.setdefault("FAKE_RCCL_TIMEOUT_MS", "30000")     # how long the stub waits for a partner before it returns an error
    env.pop("FAKE_RCCL_HOST", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "exchange_rank_checks.py")] + [str(a) for a in args], capture_output=True, text=True,
                         env=env, timeout=600, cwd=ROOT)
    print(out.stdout[-2000:])
    assert out.returncode == 0 and '"ok": true' in out.stdout, out.stdout[-2000:] + out.stderr[-6000:]


@pytest.mark.parametrize("n", [2, 4, 8, 3, 6])
def test_exchange_end_to_end_against_the_oracle(gpu, stub, n):
    """Every rank channelizes its time shard (64 x 16 for 2, 4, 8 ranks; 96 x 8 for 3 and 6; 997 + 8 n output rows, so the shards are uneven)
    with ngroups = n, the exchange regroups, and rank g holds the oracle's channelizer of the WHOLE stream restricted to its channels --
    through plans.exchange_all from one thread, Comm.exchange from n threads over redio_comm_init_all, and Comm.exchange from n threads
    over redio_comm_init_rank with one shared id."""
    child(stub, "e2e", n)


def test_exchange_end_to_end_from_u8_bytes(gpu, stub):
    """Channelizer.from_bytes(raw, ngroups = 4) per shard, exchanged: the oracle's channelizer of oracle.data_to_samples(raw)."""
    child(stub, "u8")


def test_exchange_with_ranks_that_own_no_rows(gpu, stub):
    """8 ranks and 5 output rows (three ranks own none and pass null buffers), 3 ranks and 2 rows, and the empty stream: the ranks that own
    rows still deliver to everybody, nothing is posted for the others, nothing is left unmatched."""
    child(stub, "few")


@pytest.mark.parametrize("which", ["A", "B"])
def test_exchange_pieces_with_unequal_peers(gpu, stub, which):
    """Three ranks at 64 channels per rank row (128 floats), device-filled pattern buffers compared on the device.  A: rows per rank
    2.5 * 2^20 + 3 (between two and three pieces of 2^27 floats, not a multiple), 2^20 (exactly one piece: the boundary of the `> o`
    test in xfer_group) and 0.  B: 5, 2^20 + 1 (one piece plus one row) and 0.  For every rank out[g][off[q] : off[q] + rows[q]] equals
    grouped[q][g], the words behind every output are untouched, no copy exceeded 2^27 floats and the number of copies is the sum over
    senders of ceil(rows * 128 / 2^27) times three (A: 12, B: 9).  Device memory of case A: 5.25 GiB of inputs and 3 x 1.75 GiB of
    outputs, about 11 GiB with the fill's temporary; everything is freed when the child ends."""
    child(stub, "pieces", which)


def test_exchange_at_builds_the_time_ordered_result_piece_by_piece(gpu, stub):
    """redio_pfb_exchange_at at 4 ranks: each shard analysed in two pieces of different length on one stream and exchanged piece by piece on
    a second one, out_row_offset[q] = first row of rank q + rows already sent, both analyses queued before the first exchange and only
    the caller's event between the two streams.  The assembled rows equal the oracle's."""
    child(stub, "at")


def test_exchange_leaves_device_and_rejects_bad_arguments_before_queueing(gpu, stub):
    """After an exchange from a thread whose device was set beforehand the current device is still that one.  At 3 ranks: a communicator
    list with an entry of another size or a null entry, a null d_grouped on a rank that owns rows (single and _all form), a null d_out
    with rows to receive, zero channels -> REDIO_ERR_ARG with every counter of the stub still zero and the outputs unchanged."""
    child(stub, "state")


def test_sharded_channelizer_from_one_cpp_process_at_four_ranks(gpu, stub, oracle, tmp_path):
    """tests/test_kpn_cpp.py::test_sharded_channelizer_from_one_cpp_process with KPN_C4_RANKS=4: the C++ host (one channelizer thread per
    rank, redio_comm_init_all / redio_pfb_exchange_all) with four ranks on the one device, through the stub."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "tests", "cpp"), "-s"])
    M, P, rows = 64, 16, 3001
    x = oracle.synth_iq(0x5EED0004, 0, M * rows)
    x.tofile(tmp_path / "in.bin")
    env = dict(os.environ)
    env.update(REDIO_RCCL_LIB=stub, FAKE_RCCL_TIMEOUT_MS="30000", KPN_C4_RANKS="4")
    out = subprocess.run([os.path.join(ROOT, "tests", "_build", "kpn_tests"), "devc4", str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "0"],
                         capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr
    ndev = int(out.stdout.split("devices")[1].split()[0])
    assert ndev == 4
    want = oracle.pfb_channelizer(x, oracle.lpf_corrected(M * P, 0.45 / M), M, P, True)
    cpg, nout = M // ndev, rows - P + 1
    assert nout % ndev
    got = np.fromfile(tmp_path / "out.bin", dtype=np.complex64).reshape(ndev, nout, cpg)
    for g in range(ndev):
        assert np.array_equal(np.ascontiguousarray(got[g]).view(np.uint32), np.ascontiguousarray(want[:, g * cpg:(g + 1) * cpg]).view(np.uint32)), g
