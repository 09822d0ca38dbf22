// fake_rccl.cpp -- a stub transport for libredio_amd/csrc/comm.hip (test infrastructure; loaded only through REDIO_RCCL_LIB).
// It exports the nine nccl* entry points comm.hip resolves and lets ALL ranks of a communicator live on ONE device (or on none),
// so that the exchange's buffer arithmetic, its pairing of sends and receives across ranks and pieces, its argument handling and
// the device state it leaves can be run with 2 to 8 ranks on a one-GPU box.  It proves nothing about RCCL itself.
//
// ncclSend / ncclRecv inside a group are only recorded.  The outermost ncclGroupEnd queues them per ordered pair (source rank,
// destination rank), matches them first in first out, and issues one device-to-device hipMemcpyAsync per matched pair, ordered by
// events after everything already queued on the sender's and on the receiver's stream and before everything queued later on either.
// With one rank per thread the group then waits on the host (FAKE_RCCL_TIMEOUT_MS, default 60000) until every operation of the group
// has met its partner; the thread that arrives second issues the copy.  When the limit expires the group's unmatched operations
// are withdrawn and ncclSystemError is returned: a mismatch is an error, never a hang.
// The stub is strict: ncclInvalidUsage for a send or receive outside a group and for a group end without a start;
// ncclInvalidArgument for a peer outside 0 .. nranks-1, a null buffer with a count, and a matched pair whose counts or types differ.
// FAKE_RCCL_HOST=1: the copy is memcpy and no HIP call is made (the matching logic on a machine without a GPU).
// Counters for the tests: fake_rccl_copies / _max_count / _unmatched / _errors / _zero_copies, fake_rccl_reset.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <unistd.h>
#include <vector>

namespace {
const char ID_MAGIC[16] = "fake_rccl-id";

struct GroupCtx { // one outermost group of one thread
    size_t outstanding = 0;
    ncclResult_t error = ncclSuccess;
    std::string detail;
};
struct Op {
    void *ptr;
    size_t count;
    ncclDataType_t type;
    hipStream_t stream;
    std::shared_ptr<GroupCtx> grp;
};
struct World { // the ranks that share one unique id (or one ncclCommInitAll)
    int nranks = 0;
    int alive = 0;
    std::vector<char> joined;
    std::string id;
    std::vector<std::deque<Op>> sends, recvs; // [src * nranks + dst]
};
} // namespace

struct ncclComm { // the handle behind ncclComm_t
    std::shared_ptr<World> world;
    int rank, device;
};

namespace {
struct Rec { ncclComm *comm; bool send; int peer; void *ptr; size_t count; ncclDataType_t type; hipStream_t stream; };

std::mutex g_mu;
std::condition_variable g_cv;
std::map<std::string, std::shared_ptr<World>> g_worlds; // by unique id, while ranks are still joining or alive
std::vector<World *> g_live;                            // every world that still has a communicator
unsigned long long g_copies, g_max_count, g_withdrawn, g_errors, g_zero_copies, g_ids;

thread_local int t_depth = 0;
thread_local std::vector<Rec> t_recs;
thread_local ncclResult_t t_group_error = ncclSuccess; // the first error of a call inside the open group: ncclGroupEnd reports it too
thread_local char t_detail[256] = "";
thread_local char t_text[320] = "";

bool host_mode()
{
    static const bool h = [] { const char *e = getenv("FAKE_RCCL_HOST"); return e && *e && strcmp(e, "0") != 0; }();
    return h;
}
long timeout_ms()
{
    static const long t = [] { const char *e = getenv("FAKE_RCCL_TIMEOUT_MS"); const long v = e ? atol(e) : 0; return v > 0 ? v : 60000L; }();
    return t;
}
size_t type_bytes(ncclDataType_t t)
{
    switch (t) {
    case ncclInt8: case ncclUint8: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
    }
}
// every error the stub returns goes through here (g_mu NOT held)
ncclResult_t fail(ncclResult_t e, const char *detail)
{
    snprintf(t_detail, sizeof t_detail, "%s", detail);
    std::lock_guard<std::mutex> lk(g_mu);
    ++g_errors;
    return e;
}
ncclResult_t hip_fail(hipError_t e, const char *what)
{
    char b[200];
    snprintf(b, sizeof b, "%s: %s", what, hipGetErrorString(e));
    return fail(ncclUnhandledCudaError, b);
}

// the copy of one matched pair (g_mu held: copies of one pair of streams are issued in matching order)
hipError_t issue_copy(const Op &s, const Op &r, int src_dev, int dst_dev)
{
    const size_t bytes = s.count * type_bytes(s.type);
    ++g_copies;
    if (s.count > g_max_count) g_max_count = s.count;
    if (bytes == 0) { ++g_zero_copies; return hipSuccess; }
    if (host_mode()) { memcpy(r.ptr, s.ptr, bytes); return hipSuccess; }
    (void)src_dev;
    int prev = -1;
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    hipError_t e = hipSetDevice(dst_dev);
    hipEvent_t sent = nullptr, done = nullptr;
    const bool two = s.stream != r.stream;
    if (e == hipSuccess && two) { // the receiver's stream waits for what the sender's stream holds so far
        e = hipEventCreateWithFlags(&sent, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(sent, s.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(r.stream, sent, 0);
    }
    if (e == hipSuccess) e = hipMemcpyAsync(r.ptr, s.ptr, bytes, hipMemcpyDeviceToDevice, r.stream);
    if (e == hipSuccess && two) { // and the sender's later work waits for the copy
        e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(done, r.stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(s.stream, done, 0);
    }
    if (sent) (void)hipEventDestroy(sent); // a recorded event is released once it has completed
    if (done) (void)hipEventDestroy(done);
    if (prev >= 0) (void)hipSetDevice(prev);
    return e;
}

void settle(const std::shared_ptr<GroupCtx> &g, ncclResult_t e, const char *detail)
{
    if (g->outstanding) --g->outstanding;
    if (e != ncclSuccess && g->error == ncclSuccess) { g->error = e; g->detail = detail; }
}

// match what the queues of pair (src, dst) hold, first in first out (g_mu held)
void match_pair(ncclComm *c, int src, int dst)
{
    World &w = *c->world;
    std::deque<Op> &sq = w.sends[(size_t)src * w.nranks + dst], &rq = w.recvs[(size_t)src * w.nranks + dst];
    while (!sq.empty() && !rq.empty()) {
        const Op s = sq.front(), r = rq.front();
        sq.pop_front(); rq.pop_front();
        ncclResult_t e = ncclSuccess;
        char d[200] = "";
        if (s.count != r.count || s.type != r.type) {
            e = ncclInvalidArgument;
            snprintf(d, sizeof d, "rank %d sends %zu elements of type %d to rank %d, which receives %zu of type %d", src, s.count, (int)s.type, dst,
                     r.count, (int)r.type);
        } else {
            const hipError_t he = issue_copy(s, r, c->device, c->device);
            if (he != hipSuccess) { e = ncclUnhandledCudaError; snprintf(d, sizeof d, "copy %d -> %d: %s", src, dst, hipGetErrorString(he)); }
        }
        settle(s.grp, e, d);
        if (r.grp != s.grp) settle(r.grp, e, d); else if (r.grp->outstanding) --r.grp->outstanding;
    }
}

size_t withdraw(World &w, const std::shared_ptr<GroupCtx> &g)
{
    size_t n = 0;
    for (std::vector<std::deque<Op>> *qs : {&w.sends, &w.recvs})
        for (std::deque<Op> &q : *qs)
            for (auto it = q.begin(); it != q.end();)
                if (it->grp == g) { it = q.erase(it); ++n; } else ++it;
    return n;
}

std::shared_ptr<World> new_world(int nranks) // g_mu held
{
    auto w = std::make_shared<World>();
    g_live.push_back(w.get());
    w->nranks = nranks;
    w->joined.assign((size_t)nranks, 0);
    w->sends.resize((size_t)nranks * nranks);
    w->recvs.resize((size_t)nranks * nranks);
    return w;
}

ncclResult_t record(bool send, const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    ncclResult_t e = ncclSuccess;
    char d[160] = "";
    const char *what = send ? "ncclSend" : "ncclRecv";
    if (!comm) { e = ncclInvalidArgument; snprintf(d, sizeof d, "%s: null communicator", what); }
    else if (t_depth == 0) { e = ncclInvalidUsage; snprintf(d, sizeof d, "%s outside a group", what); }
    else if (peer < 0 || peer >= comm->world->nranks) { e = ncclInvalidArgument; snprintf(d, sizeof d, "%s: peer %d outside 0 .. %d", what, peer, comm->world->nranks - 1); }
    else if (type_bytes(type) == 0) { e = ncclInvalidArgument; snprintf(d, sizeof d, "%s: data type %d", what, (int)type); }
    else if (count && !buf) { e = ncclInvalidArgument; snprintf(d, sizeof d, "%s: null buffer with %zu elements", what, count); }
    if (e != ncclSuccess) {
        if (t_depth && t_group_error == ncclSuccess) t_group_error = e;
        return fail(e, d);
    }
    t_recs.push_back({comm, send, peer, const_cast<void *>(buf), count, type, stream});
    return ncclSuccess;
}
} // namespace

extern "C" {
ncclResult_t ncclGetUniqueId(ncclUniqueId *id)
{
    if (!id) return fail(ncclInvalidArgument, "ncclGetUniqueId: null id");
    memset(id, 0, sizeof *id);
    memcpy(id->internal, ID_MAGIC, sizeof ID_MAGIC);
    unsigned long long n;
    { std::lock_guard<std::mutex> lk(g_mu); n = ++g_ids; }
    snprintf(id->internal + sizeof ID_MAGIC, sizeof id->internal - sizeof ID_MAGIC, "%ld-%llu", (long)getpid(), n);
    return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank)
{
    if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(ncclInvalidArgument, "ncclCommInitRank: arguments");
    if (memcmp(id.internal, ID_MAGIC, sizeof ID_MAGIC) != 0) return fail(ncclInvalidArgument, "ncclCommInitRank: not an id of ncclGetUniqueId");
    int dev = 0;
    if (!host_mode()) { const hipError_t he = hipGetDevice(&dev); if (he != hipSuccess) return hip_fail(he, "hipGetDevice"); }
    const char *why = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const std::string key(id.internal, sizeof id.internal);
        std::shared_ptr<World> &w = g_worlds[key];
        if (!w) { w = new_world(nranks); w->id = key; }
        if (w->nranks != nranks) why = "ncclCommInitRank: another rank joined this id with a different nranks";
        else if (w->joined[(size_t)rank]) why = "ncclCommInitRank: this rank of the id has joined already";
        else {
            w->joined[(size_t)rank] = 1;
            ++w->alive;
            *comm = new ncclComm{w, rank, dev};
        }
    }
    return why ? fail(ncclInvalidArgument, why) : ncclSuccess;
}

// the same device may appear several times: that is what the stub is for
ncclResult_t ncclCommInitAll(ncclComm_t *comms, int ndev, const int *devlist)
{
    if (!comms || ndev < 1) return fail(ncclInvalidArgument, "ncclCommInitAll: arguments");
    int have = 0;
    if (!host_mode()) {
        const hipError_t he = hipGetDeviceCount(&have);
        if (he != hipSuccess) return hip_fail(he, "hipGetDeviceCount");
        for (int i = 0; i < ndev; ++i)
            if (devlist && (devlist[i] < 0 || devlist[i] >= have)) return fail(ncclInvalidArgument, "ncclCommInitAll: no such device");
    }
    std::lock_guard<std::mutex> lk(g_mu);
    std::shared_ptr<World> w = new_world(ndev);
    w->alive = ndev;
    for (int i = 0; i < ndev; ++i) comms[i] = new ncclComm{w, i, devlist ? devlist[i] : (host_mode() ? 0 : i % (have ? have : 1))};
    return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm)
{
    if (!comm) return ncclSuccess;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        World &w = *comm->world;
        // what this rank posted and nobody met: its sends (src == rank) and its receives (dst == rank)
        for (int q = 0; q < w.nranks; ++q) {
            std::deque<Op> &s = w.sends[(size_t)comm->rank * w.nranks + q], &r = w.recvs[(size_t)q * w.nranks + comm->rank];
            g_withdrawn += s.size() + r.size();
            for (std::deque<Op> *dq : {&s, &r})
                for (Op &o : *dq) settle(o.grp, ncclInvalidUsage, "communicator destroyed under an unmatched operation");
            s.clear(); r.clear();
        }
        if (--w.alive == 0) {
            for (auto it = g_live.begin(); it != g_live.end(); ++it)
                if (*it == &w) { g_live.erase(it); break; }
            if (!w.id.empty()) g_worlds.erase(w.id); // comm still holds the world until it is deleted below
        }
    }
    g_cv.notify_all();
    delete comm;
    return ncclSuccess;
}

ncclResult_t ncclSend(const void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    return record(true, buf, count, type, peer, comm, stream);
}
ncclResult_t ncclRecv(void *buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream)
{
    return record(false, buf, count, type, peer, comm, stream);
}

ncclResult_t ncclGroupStart()
{
    if (t_depth++ == 0) { t_recs.clear(); t_group_error = ncclSuccess; }
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd()
{
    if (t_depth == 0) return fail(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart");
    if (--t_depth) return ncclSuccess;
    std::vector<Rec> recs;
    recs.swap(t_recs);
    if (t_group_error != ncclSuccess) { // a refused call inside the group: nothing of the group is issued
        snprintf(t_detail, sizeof t_detail, "a call inside the group was refused");
        return t_group_error;
    }
    if (recs.empty()) return ncclSuccess;
    auto grp = std::make_shared<GroupCtx>();
    grp->outstanding = recs.size();
    ncclResult_t e = ncclSuccess;
    std::string detail;
    {
        std::unique_lock<std::mutex> lk(g_mu);
        for (const Rec &r : recs) {
            World &w = *r.comm->world;
            const int src = r.send ? r.comm->rank : r.peer, dst = r.send ? r.peer : r.comm->rank;
            (r.send ? w.sends : w.recvs)[(size_t)src * w.nranks + dst].push_back({r.ptr, r.count, r.type, r.stream, grp});
        }
        for (const Rec &r : recs) match_pair(r.comm, r.send ? r.comm->rank : r.peer, r.send ? r.peer : r.comm->rank);
        g_cv.notify_all();
        const bool met = g_cv.wait_for(lk, std::chrono::milliseconds(timeout_ms()), [&] { return grp->outstanding == 0; });
        if (!met) {
            size_t n = 0;
            std::vector<World *> seen;
            for (const Rec &r : recs) {
                World *w = r.comm->world.get();
                bool dup = false;
                for (World *s : seen) dup = dup || s == w;
                if (!dup) { seen.push_back(w); n += withdraw(*w, grp); }
            }
            g_withdrawn += n;
            char d[160];
            snprintf(d, sizeof d, "%zu operation(s) of the group found no partner within %ld ms", n, timeout_ms());
            if (grp->error == ncclSuccess) { grp->error = ncclSystemError; grp->detail = d; }
        }
        e = grp->error;
        detail = grp->detail;
    }
    return e == ncclSuccess ? ncclSuccess : fail(e, detail.c_str());
}

const char *ncclGetErrorString(ncclResult_t e)
{
    const char *name = "unknown result code";
    switch (e) {
    case ncclSuccess: return "no error";
    case ncclUnhandledCudaError: name = "unhandled cuda error"; break;
    case ncclSystemError: name = "unhandled system error"; break;
    case ncclInternalError: name = "internal error"; break;
    case ncclInvalidArgument: name = "invalid argument"; break;
    case ncclInvalidUsage: name = "invalid usage"; break;
    default: break;
    }
    snprintf(t_text, sizeof t_text, "fake_rccl: %s (%s)", name, t_detail);
    return t_text;
}

// ---- what the tests read ----
unsigned long long fake_rccl_copies(void) { std::lock_guard<std::mutex> lk(g_mu); return g_copies; }          // matched pairs whose copy was issued
unsigned long long fake_rccl_zero_copies(void) { std::lock_guard<std::mutex> lk(g_mu); return g_zero_copies; } // ... of them with a count of zero
unsigned long long fake_rccl_max_count(void) { std::lock_guard<std::mutex> lk(g_mu); return g_max_count; }    // elements of the largest copy
unsigned long long fake_rccl_errors(void) { std::lock_guard<std::mutex> lk(g_mu); return g_errors; }          // calls that returned an error
// operations that never met a partner: withdrawn at a time-out, dropped with their communicator, or still queued now
unsigned long long fake_rccl_unmatched(void)
{
    std::lock_guard<std::mutex> lk(g_mu);
    unsigned long long n = g_withdrawn;
    for (const World *w : g_live)
        for (const std::vector<std::deque<Op>> *qs : {&w->sends, &w->recvs})
            for (const std::deque<Op> &q : *qs) n += q.size();
    return n;
}
const char *fake_rccl_id_magic(void) { return ID_MAGIC; }
int fake_rccl_host_mode(void) { return host_mode() ? 1 : 0; }
void fake_rccl_reset(void) { std::lock_guard<std::mutex> lk(g_mu); g_copies = g_max_count = g_withdrawn = g_errors = g_zero_copies = 0; }
}
