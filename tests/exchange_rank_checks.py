#!/usr/bin/env python3
"""Children of tests/test_gpu_exchange_ranks.py: the channelizer's exchange (libredio_amd/csrc/comm.hip) at 2 to 8 ranks that all live
on ONE device, through the stub transport the parent names in REDIO_RCCL_LIB (tests/stub/fake_rccl.cpp).  One case per process,
because a transport is loaded once per process.  Every comparison is bit for bit.

    python tests/exchange_rank_checks.py e2e N          N ranks, uneven shards, all three entry points, against the oracle
    python tests/exchange_rank_checks.py u8             the same from u8 I/Q bytes (Channelizer.from_bytes, ngroups = 4)
    python tests/exchange_rank_checks.py few            8 ranks and 5 rows; the empty stream
    python tests/exchange_rank_checks.py pieces A|B     messages of several 2^27-float pieces with unequal peers
    python tests/exchange_rank_checks.py at             redio_pfb_exchange_at: shards analysed and exchanged in two pieces
    python tests/exchange_rank_checks.py state          device state and argument errors at N > 1

Prints {"ok": true} and exits 0 once every check held and the stub reports no unmatched operation and no error."""
import ctypes as C
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import libredio_amd as R
import oracle as O
from libredio_amd import plans, sharding

PIECE = 1 << 27                     # comm.hip COMM_PIECE: floats per transfer
GUARD = 256                         # words behind every output that must stay as they were
GUARD_WORD = 0x7FC0BEEF             # a NaN pattern no result holds
COUNTERS = ("copies", "zero_copies", "max_count", "errors", "unmatched")
ENTRIES = ("all", "threads_init_all", "threads_init_rank")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stub():
    """The stub through its own handle: the same mapping libredio.so loaded (same file), so these are the counters of its calls."""
    L = C.CDLL(os.environ["REDIO_RCCL_LIB"])
    for n in COUNTERS:
        getattr(L, "fake_rccl_" + n).restype = C.c_ulonglong
    assert L.fake_rccl_host_mode() == 0
    return L


def counters(L):
    return {n: int(getattr(L, "fake_rccl_" + n)()) for n in COUNTERS}


def counts_are(L, **want):
    full = dict.fromkeys(COUNTERS, 0)
    full.update(want)
    got = counters(L)
    assert got == full, (got, full)


def in_threads(n, body):
    """body(rank) on one thread per rank; the first exception of any of them is raised here."""
    errs = [None] * n

    def run(r):
        try:
            torch.cuda.set_device(0)
            body(r)
        except BaseException as e:  # noqa: BLE001
            if isinstance(e, R.RedioError):             # the transport's own words are kept per calling thread
                e = RuntimeError(f"{e} [{R.lib().redio_comm_last_error().decode()}]")
            errs[r] = e
    ts = [threading.Thread(target=run, args=(r,)) for r in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for r, e in enumerate(errs):
        if e is not None:
            raise AssertionError(f"rank {r}: {e!r}") from e


def make_comms(n, how):
    """n communicators on device 0: redio_comm_init_all, or redio_comm_init_rank from n threads with one shared id."""
    if how != "threads_init_rank":
        return R.Comm.init_all([0] * n)
    buf = C.create_string_buffer(128)
    R.check(R.lib().redio_comm_unique_id(buf), "comm_unique_id")
    comms = [None] * n

    def join(r):
        h = C.c_void_p()
        R.check(R.lib().redio_comm_init_rank(C.byref(h), n, r, buf), "comm_init_rank")
        comms[r] = R.Comm(h, r, n)
    in_threads(n, join)
    assert [R.lib().redio_comm_rank(c._h) for c in comms] == list(range(n)) and all(R.lib().redio_comm_size(c._h) == n for c in comms)
    return comms


def guarded_out(rows, cpg):
    """[rows][cpg] complex64 with GUARD words behind it, every word preset; finished before any other stream can touch it."""
    buf = torch.empty(rows * cpg * 2 + GUARD, dtype=torch.int32, device="cuda")
    buf.fill_(GUARD_WORD)
    torch.cuda.synchronize()
    return buf, buf[: rows * cpg * 2].view(torch.complex64).view(rows, cpg)


def guard_intact(buf):
    return bool((buf[-GUARD:] == GUARD_WORD).all().item())


def shards(n, total_rows, P):
    sh = [sharding.channelizer_time_shard(g, n, total_rows, P) for g in range(n)]
    return [s[0] for s in sh], [s[1] for s in sh], [s[2] for s in sh]


def run_exchange(entry, n, analyse, rows, cpg):
    """Every rank analyses its shard (analyse(rank) -> [n][rows[rank]][cpg]) and the exchange regroups; returns (guard buffers, outputs)."""
    comms = make_comms(n, entry)
    held = [guarded_out(sum(rows), cpg) for _ in range(n)]
    if entry == "all":
        grouped = [analyse(g) for g in range(n)]
        plans.exchange_all(comms, grouped, rows, outs=[o for _, o in held])
        torch.cuda.synchronize()
    else:
        def rank(g):
            s = torch.cuda.Stream()                     # every rank on a stream of its own, as on its own GPU
            with torch.cuda.stream(s):
                comms[g].exchange(analyse(g), rows, out=held[g][1])
            s.synchronize()
        in_threads(n, rank)
    del comms
    return held


def e2e(L, n, M, P, nout, from_bytes=False, entries=ENTRIES):
    """Rank g must hold the oracle's channelizer of the WHOLE stream restricted to channels g * cpg .. (g + 1) * cpg."""
    total_rows = nout + P - 1 if nout else P - 1
    h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
    cpg = sharding.channelizer_exchange_layout(n, M)
    first, rows, nin = shards(n, total_rows, P)
    assert sum(rows) == nout
    if from_bytes:
        raw = np.random.default_rng(n).integers(0, 256, 2 * M * total_rows, dtype=np.uint8)
        raw[:256] = np.arange(256, dtype=np.uint8)
        want = O.pfb_channelizer(O.data_to_samples(raw), h, M, P, True)
    else:
        xs = O.synth_iq(0x5EED0004, 0, M * total_rows)
        want = O.pfb_channelizer(xs, h, M, P, True)
    want = np.asarray(want).reshape(nout, M)

    def analyse(g):
        if rows[g] == 0:                                # this rank owns no output rows: nothing to analyse, a null buffer
            return torch.empty((n, 0, cpg), dtype=torch.complex64, device="cuda")
        plan = R.Channelizer(h, M, P)
        if from_bytes:
            out = plan.from_bytes(torch.from_numpy(raw[2 * M * first[g]: 2 * M * (first[g] + nin[g])]).cuda(), ngroups=n)
        else:
            out = plan(torch.from_numpy(xs[M * first[g]: M * (first[g] + nin[g])]).cuda(), ngroups=n)
        out = out.reshape(n, -1, cpg)
        assert out.shape == (n, rows[g], cpg)
        return out

    senders = sum(1 for r in rows if r)
    for entry in entries:
        L.fake_rccl_reset()
        held = run_exchange(entry, n, analyse, rows, cpg)
        for g, (buf, out) in enumerate(held):
            got = out.cpu().numpy()
            assert got.shape == (nout, cpg)
            assert np.array_equal(bits(got), bits(want[:, g * cpg:(g + 1) * cpg])), f"{entry}: rank {g} of {n} differs from the oracle"
            assert guard_intact(buf), f"{entry}: rank {g}: the words behind its output changed"
        counts_are(L, copies=senders * n, max_count=max(rows) * cpg * 2 if senders else 0)


def case_e2e(L, n):
    M, P = (64, 16) if 64 % n == 0 else (96, 8)
    nout = 997 + 8 * n
    assert M % n == 0 and nout % n != 0                 # uneven shards
    e2e(L, n, M, P, nout)


def case_u8(L):
    e2e(L, 4, 64, 16, 1029, from_bytes=True)


def case_few(L):
    e2e(L, 8, 64, 16, 5)                                # ranks 5, 6, 7 own no rows
    e2e(L, 8, 64, 16, 0)                                # nobody owns a row: no buffer, no transfer
    e2e(L, 3, 96, 8, 2)


def pattern(view, seed):
    """device fill of an int32 view with words that differ along the buffer and between buffers"""
    view.copy_(torch.arange(view.numel(), dtype=torch.int32, device="cuda"))
    view.mul_(-1640531535).add_(seed)                   # 2654435761 as a wrapped int32: odd, so no two words of one buffer agree


def case_pieces(L, which):
    """Device-filled pattern buffers, no channelizer.  A: per-peer messages of 2.5 pieces + 3 rows, exactly one piece, and none;
    B: one piece plus one row, five rows, and none."""
    cpg, n = 64, 3
    fl = 2 * cpg
    rows_per_piece = PIECE // fl
    rows = {"A": [2 * rows_per_piece + rows_per_piece // 2 + 3, rows_per_piece, 0], "B": [5, rows_per_piece + 1, 0]}[which]
    assert rows_per_piece * fl == PIECE
    total = sum(rows)
    off = [sum(rows[:q]) for q in range(n)]
    grouped_i = [torch.empty(n * rows[g] * fl, dtype=torch.int32, device="cuda") for g in range(n)]
    for g in range(n):
        for q in range(n):
            if rows[g]:
                pattern(grouped_i[g][q * rows[g] * fl:(q + 1) * rows[g] * fl], 1000003 * (g * n + q) + 17)
    grouped = [t.view(torch.complex64).view(n, rows[g], cpg) if rows[g] else torch.empty((n, 0, cpg), dtype=torch.complex64, device="cuda")
               for g, t in enumerate(grouped_i)]
    copies = sum(-(-rows[s] * fl // PIECE) for s in range(n)) * n       # every sender's message to each of the n ranks, piece by piece
    biggest = min(max(rows) * fl, PIECE)
    held = [guarded_out(total, cpg) for _ in range(n)]
    for entry in ("all", "threads_init_all"):
        L.fake_rccl_reset()
        for buf, _ in held:
            buf.fill_(GUARD_WORD)
        torch.cuda.synchronize()
        comms = make_comms(n, entry)
        if entry == "all":
            plans.exchange_all(comms, grouped, rows, outs=[o for _, o in held])
            torch.cuda.synchronize()
        else:
            def rank(g):
                s = torch.cuda.Stream()
                with torch.cuda.stream(s):
                    comms[g].exchange(grouped[g], rows, out=held[g][1])
                s.synchronize()
            in_threads(n, rank)
        del comms
        for g, (buf, _) in enumerate(held):
            for q in range(n):
                got = buf[off[q] * fl:(off[q] + rows[q]) * fl]
                sent = grouped_i[q][g * rows[q] * fl:(g + 1) * rows[q] * fl]
                assert torch.equal(got, sent), f"{which} {entry}: rank {g} did not receive rank {q}'s rows of its channels at row {off[q]}"
            assert guard_intact(buf), f"{which} {entry}: rank {g}: the words behind its output changed"
        c = counters(L)
        assert c["max_count"] <= PIECE, c
        counts_are(L, copies=copies, max_count=biggest)


def case_at(L):
    """Each rank analyses its shard in two pieces of different length on one stream and exchanges them piece by piece on a second
    stream (redio_pfb_exchange_at), the second analysis queued before the first exchange.  The only order made between the two
    streams is the event a caller records after each analysis."""
    n, M, P, nout = 4, 64, 16, 1029
    total_rows = nout + P - 1
    h = R.dsputils.lpf_corrected(M * P, 0.45 / M)
    cpg = sharding.channelizer_exchange_layout(n, M)
    first, rows, _ = shards(n, total_rows, P)
    assert nout % n
    cut = [rows[q] // 3 + q for q in range(n)]          # rows of every rank's first piece; the second piece is the rest
    piece_rows = [[cut[q] for q in range(n)], [rows[q] - cut[q] for q in range(n)]]
    piece_first = [[first[q] for q in range(n)], [first[q] + cut[q] for q in range(n)]]
    assert all(0 < cut[q] < rows[q] and cut[q] != rows[q] - cut[q] for q in range(n))
    xs = O.synth_iq(0x5EED0004, 0, M * total_rows)
    want = O.pfb_channelizer(xs, h, M, P, True)
    comms = make_comms(n, "threads_init_rank")
    held = [guarded_out(nout, cpg) for _ in range(n)]
    L.fake_rccl_reset()

    def rank(g):
        plan = R.Channelizer(h, M, P)
        analysis, comm_s = torch.cuda.Stream(), torch.cuda.Stream()
        x = torch.from_numpy(xs[M * first[g]: M * (first[g] + rows[g] + P - 1)]).cuda()
        analysis.wait_stream(torch.cuda.current_stream())
        done, parts = [], []
        with torch.cuda.stream(analysis):
            for i in range(2):
                r0 = piece_first[i][g] - first[g]
                parts.append(plan(x[M * r0: M * (r0 + piece_rows[i][g] + P - 1)], ngroups=n).reshape(n, piece_rows[i][g], cpg))
                ev = torch.cuda.Event()
                ev.record(analysis)
                done.append(ev)
        for i in range(2):
            comm_s.wait_event(done[i])
            comms[g].exchange_at(parts[i], piece_rows[i], held[g][1], piece_first[i], stream=comm_s)
        comm_s.synchronize()
        analysis.synchronize()
    in_threads(n, rank)
    for g, (buf, out) in enumerate(held):
        assert np.array_equal(bits(out.cpu().numpy()), bits(want[:, g * cpg:(g + 1) * cpg])), f"rank {g}: the assembled rows differ from the oracle"
        assert guard_intact(buf)
    counts_are(L, copies=2 * n * n, max_count=max(max(p) for p in piece_rows) * cpg * 2)
    del comms


def case_state(L):
    lib = R.lib()
    n, cpg, rows = 3, 32, [7, 0, 4]
    comms = make_comms(n, "threads_init_all")
    grouped = [torch.view_as_complex(torch.randn((n, rows[g], cpg, 2), device="cuda")) for g in range(n)]
    held = [guarded_out(sum(rows), cpg) for _ in range(n)]
    torch.cuda.synchronize()
    L.fake_rccl_reset()
    seen = [None] * n

    def rank(g):                                        # in_threads has made device 0 current on this thread
        comms[g].exchange(grouped[g], rows, out=held[g][1])
        dev = C.c_int(-1)
        R.check(lib.redio_get_device(C.byref(dev)), "get_device")
        seen[g] = (torch.cuda.current_device(), dev.value)
        torch.cuda.synchronize()
    in_threads(n, rank)
    assert seen == [(0, 0)] * n, seen
    off = [0, 7, 7]
    for g in range(n):
        for q in range(n):
            assert torch.equal(held[g][1][off[q]: off[q] + rows[q]], grouped[q][g])
        assert guard_intact(held[g][0])
    counts_are(L, copies=2 * n, max_count=7 * cpg * 2)
    # argument errors come back before anything is queued
    L.fake_rccl_reset()
    ERR_ARG = -1
    sz, vp = C.c_size_t, C.c_void_p
    hs = lambda cs: (vp * len(cs))(*[c._h for c in cs])
    ptrs = lambda ts: (vp * len(ts))(*[t.data_ptr() if t.numel() else None for t in ts])
    outs = [o for _, o in held]
    rows_c = (sz * n)(*rows)
    other = make_comms(2, "all")
    mixed = [comms[0], other[1], comms[2]]              # one entry of the list belongs to a communicator of another size
    assert lib.redio_pfb_exchange_all(hs(mixed), n, ptrs(grouped), ptrs(outs), rows_c, cpg, None) == ERR_ARG
    assert lib.redio_pfb_exchange_all((vp * n)(comms[0]._h, comms[1]._h, None), n, ptrs(grouped), ptrs(outs), rows_c, cpg, None) == ERR_ARG
    no_send = [grouped[0], grouped[1], grouped[1]]      # rank 2 owns 4 rows and has no buffer to send from (rank 1's is null: it owns none)
    assert grouped[1].numel() == 0
    assert lib.redio_pfb_exchange_all(hs(comms), n, ptrs(no_send), ptrs(outs), rows_c, cpg, None) == ERR_ARG
    no_out = [outs[0], outs[1], grouped[1]]
    assert lib.redio_pfb_exchange_all(hs(comms), n, ptrs(grouped), ptrs(no_out), rows_c, cpg, None) == ERR_ARG
    assert lib.redio_pfb_exchange(comms[0]._h, None, outs[0].data_ptr(), rows_c, cpg, None) == ERR_ARG
    assert lib.redio_pfb_exchange(comms[1]._h, None, None, rows_c, cpg, None) == ERR_ARG          # rank 1 sends nothing but receives 11 rows
    assert lib.redio_pfb_exchange_at(comms[2]._h, None, outs[2].data_ptr(), rows_c, (sz * n)(*off), cpg, None) == ERR_ARG
    assert lib.redio_pfb_exchange(comms[0]._h, grouped[0].data_ptr(), outs[0].data_ptr(), rows_c, 0, None) == ERR_ARG
    torch.cuda.synchronize()
    counts_are(L)
    for g in range(n):                                  # and nothing was written
        for q in range(n):
            assert torch.equal(held[g][1][off[q]: off[q] + rows[q]], grouped[q][g])
    del comms, other, mixed


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    torch.cuda.set_device(0)
    L = stub()
    try:
        run_case(L, sys.argv[1])
    except R.RedioError as e:
        raise RuntimeError(f"{e} [{R.lib().redio_comm_last_error().decode()}]") from e
    import gc
    gc.collect()                                        # the communicators are destroyed: what they still held would be counted now
    c = counters(L)
    assert c["unmatched"] == 0 and c["errors"] == 0, c
    print(json.dumps({"ok": True, "stub": c}))


def run_case(L, case):
    if case == "e2e":
        case_e2e(L, int(sys.argv[2]))
    elif case == "u8":
        case_u8(L)
    elif case == "few":
        case_few(L)
    elif case == "pieces":
        case_pieces(L, sys.argv[2])
    elif case == "at":
        case_at(L)
    elif case == "state":
        case_state(L)
    else:
        raise SystemExit(f"unknown case {case}")


if __name__ == "__main__":
    main()
