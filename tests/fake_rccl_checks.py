#!/usr/bin/env python3
"""Children of tests/test_fake_rccl.py: one case per process, because a transport is loaded once per process.

    python tests/fake_rccl_checks.py all_to_all N one|threads     the stub alone (FAKE_RCCL_HOST=1), host buffers through ctypes
    python tests/fake_rccl_checks.py refuse RULE                    one rule the stub must enforce
    python tests/fake_rccl_checks.py seam ok|missing|no_symbol      libredio.so with REDIO_RCCL_LIB set by the parent

Needs no device.  Prints {"ok": true} and exits 0, else raises."""
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STUB = os.path.join(ROOT, "tests", "_build", "libfake_rccl.so")

ncclSuccess, ncclUnhandledCudaError, ncclSystemError, ncclInternalError, ncclInvalidArgument, ncclInvalidUsage = range(6)
ncclUint8, ncclInt32, ncclFloat = 1, 2, 7  # rccl.h ncclDataType_t
COUNTERS = ("copies", "zero_copies", "max_count", "errors", "unmatched")


class UniqueId(C.Structure):
    _fields_ = [("internal", C.c_char * 128)]


def load_stub(path=STUB):
    L = C.CDLL(path)
    vp, sz, i = C.c_void_p, C.c_size_t, C.c_int
    L.ncclGetUniqueId.argtypes = [C.POINTER(UniqueId)]
    L.ncclCommInitRank.argtypes = [C.POINTER(vp), i, UniqueId, i]
    L.ncclCommInitAll.argtypes = [C.POINTER(vp), i, C.POINTER(i)]
    L.ncclCommDestroy.argtypes = [vp]
    L.ncclSend.argtypes = [vp, sz, i, i, vp, vp]
    L.ncclRecv.argtypes = [vp, sz, i, i, vp, vp]
    L.ncclGetErrorString.argtypes = [i]
    L.ncclGetErrorString.restype = C.c_char_p
    L.fake_rccl_id_magic.restype = C.c_char_p
    for n in COUNTERS:
        getattr(L, "fake_rccl_" + n).restype = C.c_ulonglong
    return L


def counters(L):
    return {n: int(getattr(L, "fake_rccl_" + n)()) for n in COUNTERS}


def counts_are(L, **want):
    full = dict.fromkeys(COUNTERS, 0)
    full.update(want)
    got = counters(L)
    assert got == full, (got, full)


def init_all(L, n):
    hs = (C.c_void_p * n)()
    assert L.ncclCommInitAll(hs, n, (C.c_int * n)(*([0] * n))) == ncclSuccess   # the same device n times
    return [C.c_void_p(h) for h in hs]


def ptr(a, first=0):
    return C.c_void_p(a.ctypes.data + first * a.itemsize)


def all_to_all(L, n, form):
    """counts[s][d] floats from rank s to rank d: unequal, and a third of the pairs empty and so never posted."""
    rng = np.random.default_rng(1000 + n)
    counts = [[0 if (s * n + d) % 3 == 1 else 1 + (7 * s + 13 * d) % 29 + 100 * ((s + d) % 2) for d in range(n)] for s in range(n)]
    send = [rng.standard_normal(sum(counts[s]) + 1).astype(np.float32) for s in range(n)]
    recv = [np.full(sum(counts[s][d] for s in range(n)) + 8, np.float32(-7.0)) for d in range(n)]   # 8 guard words behind
    soff = [[sum(counts[s][:d]) for d in range(n)] for s in range(n)]
    roff = [[sum(counts[q][d] for q in range(s)) for s in range(n)] for d in range(n)]

    def post(comm, r):
        for q in range(n):
            if counts[r][q]:
                assert L.ncclSend(ptr(send[r], soff[r][q]), counts[r][q], ncclFloat, q, comm, None) == ncclSuccess
            if counts[q][r]:
                assert L.ncclRecv(ptr(recv[r], roff[r][q]), counts[q][r], ncclFloat, q, comm, None) == ncclSuccess

    if form == "one":
        comms = init_all(L, n)
        assert L.ncclGroupStart() == ncclSuccess
        for r in range(n):
            post(comms[r], r)
        assert L.ncclGroupEnd() == ncclSuccess
    else:
        uid = UniqueId()
        assert L.ncclGetUniqueId(C.byref(uid)) == ncclSuccess
        comms, rcs = [None] * n, [None] * n

        def run(r):
            h = C.c_void_p()
            rcs[r] = L.ncclCommInitRank(C.byref(h), n, uid, r)
            comms[r] = h
            if rcs[r] == ncclSuccess:
                rcs[r] = L.ncclGroupStart()
                post(h, r)
                rcs[r] = rcs[r] or L.ncclGroupEnd()
        ts = [threading.Thread(target=run, args=(r,)) for r in range(n)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert rcs == [ncclSuccess] * n, rcs
    for d in range(n):
        for s in range(n):
            got, want = recv[d][roff[d][s]: roff[d][s] + counts[s][d]], send[s][soff[s][d]: soff[s][d] + counts[s][d]]
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (s, d)
        assert np.all(recv[d][-8:] == np.float32(-7.0)), f"rank {d}: the words behind its receive buffer changed"
    pairs = sum(1 for s in range(n) for d in range(n) if counts[s][d])
    assert 0 < pairs < n * n
    counts_are(L, copies=pairs, max_count=max(max(r) for r in counts))
    for h in comms:
        assert L.ncclCommDestroy(h) == ncclSuccess
    assert counters(L)["unmatched"] == 0
    L.fake_rccl_reset()
    counts_are(L)


def refuse(L, rule):
    a, b = np.arange(1, 17, dtype=np.float32), np.zeros(16, np.float32)
    c0, c1 = init_all(L, 2)
    if rule in ("count", "type"):       # a matched pair that disagrees: refused, nothing copied, both operations consumed
        assert L.ncclGroupStart() == ncclSuccess
        assert L.ncclSend(ptr(a), 16, ncclFloat, 1, c0, None) == ncclSuccess
        assert L.ncclRecv(ptr(b), 12 if rule == "count" else 16, ncclFloat if rule == "count" else ncclInt32, 0, c1, None) == ncclSuccess
        assert L.ncclGroupEnd() == ncclInvalidArgument
        assert not b.any()
        counts_are(L, errors=1)
        assert b"receives" in L.ncclGetErrorString(ncclInvalidArgument)
    elif rule == "peer":                # a peer outside 0 .. nranks - 1: refused at the call, and the group with it
        assert L.ncclGroupStart() == ncclSuccess
        assert L.ncclSend(ptr(a), 16, ncclFloat, 2, c0, None) == ncclInvalidArgument
        assert L.ncclRecv(ptr(b), 16, ncclFloat, -1, c1, None) == ncclInvalidArgument
        assert L.ncclSend(ptr(a), 16, ncclFloat, 1, c0, None) == ncclSuccess     # a good pair of the same group is not issued either
        assert L.ncclRecv(ptr(b), 16, ncclFloat, 0, c1, None) == ncclSuccess
        assert L.ncclGroupEnd() == ncclInvalidArgument
        assert not b.any()
        counts_are(L, errors=2)
    elif rule == "no_group":            # a send or a receive outside a group
        assert L.ncclSend(ptr(a), 16, ncclFloat, 1, c0, None) == ncclInvalidUsage
        assert L.ncclRecv(ptr(b), 16, ncclFloat, 0, c1, None) == ncclInvalidUsage
        assert not b.any()
        counts_are(L, errors=2)
    elif rule == "end_without_start":
        assert L.ncclGroupEnd() == ncclInvalidUsage
        assert L.ncclGroupStart() == ncclSuccess and L.ncclGroupStart() == ncclSuccess     # groups nest: only the outermost end acts
        assert L.ncclGroupEnd() == ncclSuccess and L.ncclGroupEnd() == ncclSuccess
        assert L.ncclGroupEnd() == ncclInvalidUsage
        counts_are(L, errors=2)
    elif rule == "timeout":             # a send whose receive never comes: an error after FAKE_RCCL_TIMEOUT_MS (about 1 s here), never a hang
        assert 0 < int(os.environ["FAKE_RCCL_TIMEOUT_MS"]) <= 2000
        t0 = time.monotonic()
        assert L.ncclGroupStart() == ncclSuccess
        assert L.ncclSend(ptr(a), 16, ncclFloat, 1, c0, None) == ncclSuccess
        assert L.ncclSend(ptr(a), 16, ncclFloat, 0, c0, None) == ncclSuccess     # this one has its partner and is delivered
        assert L.ncclRecv(ptr(b), 16, ncclFloat, 0, c0, None) == ncclSuccess
        assert L.ncclGroupEnd() == ncclSystemError
        assert 0.5 < time.monotonic() - t0 < 30
        assert np.array_equal(a, b)
        counts_are(L, copies=1, max_count=16, errors=1, unmatched=1)
        assert b"no partner" in L.ncclGetErrorString(ncclSystemError)
        # the withdrawn send is gone: a receive posted now finds nothing and times out too
        assert L.ncclGroupStart() == ncclSuccess
        assert L.ncclRecv(ptr(b), 16, ncclFloat, 0, c1, None) == ncclSuccess
        assert L.ncclGroupEnd() == ncclSystemError
        counts_are(L, copies=1, max_count=16, errors=2, unmatched=2)
    elif rule == "destroyed":           # operations still unmatched when their communicator is destroyed are counted
        rc = []

        def waiter():
            L.ncclGroupStart()
            L.ncclRecv(ptr(b), 16, ncclFloat, 0, c1, None)
            rc.append(L.ncclGroupEnd())
        t = threading.Thread(target=waiter)
        t.start()
        for _ in range(500):            # until the receive is queued
            if counters(L)["unmatched"] == 1:
                break
            time.sleep(0.01)
        assert counters(L)["unmatched"] == 1
        assert L.ncclCommDestroy(c1) == ncclSuccess
        t.join(20)
        assert not t.is_alive() and rc == [ncclInvalidUsage], rc
        counts_are(L, errors=1, unmatched=1)
        c1 = None
    elif rule == "join":                # ranks of one id must agree on nranks and be distinct
        uid, h = UniqueId(), C.c_void_p()
        assert L.ncclGetUniqueId(C.byref(uid)) == ncclSuccess
        assert uid.internal.startswith(L.fake_rccl_id_magic())
        assert L.ncclCommInitRank(C.byref(h), 3, uid, 0) == ncclSuccess
        h2 = C.c_void_p()
        assert L.ncclCommInitRank(C.byref(h2), 3, uid, 0) == ncclInvalidArgument
        assert L.ncclCommInitRank(C.byref(h2), 4, uid, 1) == ncclInvalidArgument
        assert L.ncclCommInitRank(C.byref(h2), 3, uid, 3) == ncclInvalidArgument
        assert L.ncclCommInitRank(C.byref(h2), 3, UniqueId(), 1) == ncclInvalidArgument   # not an id of ncclGetUniqueId
        assert L.ncclCommDestroy(h) == ncclSuccess
        counts_are(L, errors=4)
    else:
        raise SystemExit(f"unknown rule {rule}")
    for h in (c0, c1):
        if h is not None:
            assert L.ncclCommDestroy(h) == ncclSuccess


def seam(what):
    """libredio.so resolves its transport before it touches HIP, so this needs no device."""
    import libredio_amd as R
    L = R.lib()
    path = os.environ["REDIO_RCCL_LIB"]
    buf = C.create_string_buffer(128)
    rc = L.redio_comm_unique_id(buf)
    if what == "ok":
        assert rc == 0, (rc, L.redio_comm_last_error())
        stub = load_stub(path)          # the same mapping (same file): its id counter shows that the call went through it
        assert buf.raw.startswith(stub.fake_rccl_id_magic()), buf.raw[:32]
        uid = UniqueId()
        assert stub.ncclGetUniqueId(C.byref(uid)) == ncclSuccess
        serial = lambda raw: raw.rstrip(b"\0").split(b"-")[-1]
        assert serial(buf.raw) == b"1" and serial(bytes(uid)) == b"2", (buf.raw[:40], bytes(uid)[:40])
        assert not hasattr(C.CDLL(None), "fake_rccl_copies"), "the override was loaded into the global namespace"   # RTLD_LOCAL
    else:
        REDIO_ERR_COMM = -7
        assert rc == REDIO_ERR_COMM, rc
        text = L.redio_comm_last_error().decode()
        assert path in text, text
        assert ("lacks ncclGetUniqueId" if what == "no_symbol" else "not loadable") in text, text
        hs = (C.c_void_p * 2)()         # every redio_comm_* call fails the same way: no silent fall back to the real library
        assert L.redio_comm_init_all(hs, 2, None) == REDIO_ERR_COMM and path in L.redio_comm_last_error().decode()
        h = C.c_void_p()
        assert L.redio_comm_init_rank(C.byref(h), 1, 0, buf) == REDIO_ERR_COMM and path in L.redio_comm_last_error().decode()
        assert not h.value and not hs[0] and not hs[1]


def main():
    mode = sys.argv[1]
    if mode == "all_to_all":
        assert os.environ.get("FAKE_RCCL_HOST") == "1"
        L = load_stub()
        assert L.fake_rccl_host_mode() == 1
        all_to_all(L, int(sys.argv[2]), sys.argv[3])
    elif mode == "refuse":
        assert os.environ.get("FAKE_RCCL_HOST") == "1"
        refuse(load_stub(), sys.argv[2])
    elif mode == "seam":
        seam(sys.argv[2])
    else:
        raise SystemExit(f"unknown mode {mode}")
    print(json.dumps({"ok": True}))


if __name__ == "__main__":
    main()
