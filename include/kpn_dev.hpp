// kpn_dev.hpp -- device-resident messages for kpn graphs: the steps either side of
// every hot block without host round trips.  A message is a kpn::dev::View = shared ownership of a
// device buffer + (offset, length) in samples, so the reshaping blocks of src/kpn/src/kpn.rs become
// metadata operations:
//   fork (kpn.rs:182-189)            clones the handle, not the samples (kpn::fork works unchanged on Views)
//   shaper (kpn.rs:278-282)          dev::shaper: re-chunks a stream of Views into Views of length l,
//                                    zero-copy when a chunk lies inside one buffer
//   unpacketizer / shaper_vecs       the inverse is the identity on a View stream
// and the hot blocks consume and produce Views through the device plans of include/redio.h.
//
// How a message travels (round 6; before, every block did hipMalloc + hipStreamSynchronize + hipFree per message and the graph ran at
// 5 % of the bare launch rate at 2^24-sample messages, profiles/r06_kpn_graph.txt):
//   * ORDER is the GPU queue's, not the host's.  The compute blocks of a graph enqueue on ONE HIP stream per device (graph_stream()):
//     a consumer receives a message only after its producer has enqueued the work that fills it, so its own work lands behind it in the
//     same queue -- no event, no wait, no packet beyond the kernels themselves.  The kernels here fill the chip and are bound by HBM, so
//     two of them side by side would only share the bandwidth; the host threads still overlap their launch work.  Blocks that move data
//     over PCIe or synchronise with the host (to_device, to_host, the mono resample) own a private stream so that a copy never sits in front of
//     a kernel; set_stream_policy(PER_BLOCK) gives every block its own (graphs whose branches are many small kernels).
//     Between DIFFERENT streams the order is made on demand, by the side that needs it: a buffer remembers the stream that wrote it
//     and the streams that read it; a consumer on another stream records an event on the WRITER's stream at that moment (everything
//     enqueued there so far, a superset of the message's work) and makes its own stream wait for it (redio_stream_wait_event: a
//     queue-side dependency, the host thread does not block); a recycled buffer's new writer does the same with its previous readers.
//     Host synchronisation is left where data really goes to the CPU.  set_host_sync(true) restores a host synchronisation before
//     every send (debugging: a fault then belongs to the block that reports it).
//   * MEMORY is a bounded ring per block (dev::Ring): at most `depth` output buffers, recycled when the last handle to a message
//     drops; a producer whose `depth` buffers are all still held downstream WAITS in acquire() -- that is the credit scheme SURVEY.md 8b
//     asks for (the reference's unbounded mpsc has no back-pressure: a documented deviation).  After warm-up a graph performs no device
//     allocation and no hipFree (redio_malloc_count() stays put; tests/test_kpn_cpp.py).  A sink that hoards more than `depth`
//     messages of one producer without dropping them stalls that producer: drop handles, or give that block a deeper ring.
//     A ring also has a BYTE budget (default_ring_bytes_ref below): with the compute blocks on one stream, a producer that runs k
//     messages ahead puts k outputs between a message and the kernel that reads it, and rotates k + 1 buffers -- past the last-level
//     cache both cost time (measured: 6 us each on a 128 MiB message that takes 69 us with neither).
//     The rings bound MEMORY, not how far the host threads run ahead of the GPU: a buffer is recycled when its handles drop (the queue
//     orders the reuse), so hundreds of messages' kernels may sit in the HIP queue; a block that needs a result on the CPU synchronises.
//   * Blocks written elsewhere use the same three calls: `auto o = ring.acquire<T>(n, st)`, `{ Reading<T> in(view, st); enqueue...; }`,
//     `publish(o, st)` before sending o, with `BlockStream st;`.
#pragma once
#include "kpn.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <complex>
#include <map>
#include <memory>
#include <vector>

namespace kpn {
namespace dev {

inline void check(int rc)
{
    if (rc != REDIO_OK) throw std::runtime_error(redio_strerror(rc));
}

// The device calls the rings and the ordering need.  A table so that their logic (credits, recycling, who waits for whom, hand-over
// between threads) also runs where there is no GPU: tests/cpp/kpn_tests.cpp `plumbing` swaps in host memory and counting stand-ins
// and runs it under ThreadSanitizer / AddressSanitizer.  Product code never touches it: the default is libredio's C ABI.
struct DeviceApi {
    int (*malloc_)(void **, size_t) = redio_malloc;
    int (*free_)(void *) = redio_free;
    int (*event_create)(void **) = redio_event_create_sync;
    int (*event_destroy)(void *) = redio_event_destroy;
    int (*event_record)(void *, void *) = redio_event_record;
    int (*stream_wait_event)(void *, void *) = redio_stream_wait_event;
    int (*stream_create)(void **) = redio_stream_create;
    int (*stream_destroy)(void *) = redio_stream_destroy;
    int (*stream_sync)(void *) = redio_stream_sync;
    int (*get_device)(int *) = redio_get_device;
};
inline DeviceApi &api()
{
    static DeviceApi a;
    return a;
}

inline std::atomic<bool> &host_sync_flag()
{
    static std::atomic<bool> f{false};
    return f;
}
inline void set_host_sync(bool on) { host_sync_flag().store(on); }
inline std::atomic<size_t> &default_ring_depth_ref()
{
    static std::atomic<size_t> d{4};
    return d;
}
// buffers per block ring for the blocks below: >= 1 bounded (credits); 0 = no pooling, one allocation per message (the round-5 behaviour,
// kept for the before/after measurement of `kpn_tests bench_c2`)
inline void set_default_ring_depth(size_t d) { default_ring_depth_ref().store(d); }
// bytes one ring may have out with the blocks downstream (beyond the first message, which always goes).  Blocks that share the graph
// stream run in the order their threads enqueued, so a producer that runs k messages ahead puts k outputs between a message and the
// kernel that reads it and writes k + 1 buffers in rotation: past the last-level cache (256 MB of Infinity Cache on MI355X) the pair
// "transform, then checksum of its output" takes 80-82 us per 128 MiB message with the reader one or more messages behind, 75 us with
// the reader directly behind, 69 us when in addition the writer gets back the buffer just read (tools/out_buffer_reuse.py; in the
// kernel trace it is the WRITER that runs 45 instead of 52 us, the reader takes 24.5 us throughout).  Half of that cache, measured
// (profiles/r06_kpn_ring_bytes.txt): 2^24-sample messages through dev::fft run at 107 % of the bare launches (which rotate four
// buffers) with one 128 MiB output out, at 92 % with two or four; small messages keep the full depth, which hides the host threads,
// and so do messages larger than the cache, i.e. twice the budget (nothing keeps those there; measured equal or 1-3 % better unbounded);
// a message between the budget and the cache goes out alone.
inline std::atomic<size_t> &default_ring_bytes_ref()
{
    static std::atomic<size_t> b{(size_t)128 << 20};
    return b;
}
inline void set_default_ring_bytes(size_t b) { default_ring_bytes_ref().store(b); }
// Coalescing in dev::fir_fft_chain and dev::fft: after a block receives a message it also takes, without waiting, up to limit - 1 more
// that are already queued in its channel, and runs them as ONE list launch (redio_*_enqueue_list) into one ring buffer; the outputs go
// out as views of that buffer, in order, with their boundaries and bits unchanged.  A launch has a floor of about 10 us however little
// it does (profiles/r06_kpn_graph.txt: one chain launch per message costs 9.6-10.5 us from 2^13 to 2^20 input samples), which is
// all a small message costs.  1 (the default) is one launch per message.
inline std::atomic<size_t> &coalesce_limit_ref()
{
    static std::atomic<size_t> n{1};
    return n;
}
inline void set_coalesce_limit(size_t n) { coalesce_limit_ref().store(n ? n : 1); }
// ... and a batch stops growing once its messages hold this many input samples together: about one launch that fills the chip
// (2^20 samples of the 127 / 5 chain are 204 blocks, one wave each on 256 CUs).  Measured with 32 messages per list
// (profiles/r07_list_launch.txt): the graph runs 19x / 14x / 3.7x faster with coalescing at 2^13 / 2^16 / 2^18-sample messages and
// within 3 % at 2^20 and above, where a batch holds one message.  The bare list launches still gain there (2^20: 2.2 against 10.5 us
// per message, 2^24: 32 against 42 us), so this bound is a starting point: raising it is measured together with the default.
constexpr size_t COALESCE_MAX_IN = (size_t)1 << 20;

// The byte budget is a preference about ORDER, never a reason to stop: a consumer that keeps a message while it waits for the next one
// (a block with memory of its own) would otherwise wait for ever on a producer held back by its budget.  A budget wait that lasts this
// long ends with the message going out anyway (a consumer that sat in a long host synchronisation with a message in hand: once); after
// three such waits in a row the ring stops using its budget, and only `depth` bounds it from then on, as it always did.
inline std::atomic<int> &ring_patience_ms_ref()
{
    static std::atomic<int> ms{50};
    return ms;
}
inline void set_ring_patience_ms(int ms) { ring_patience_ms_ref().store(ms); }
inline std::atomic<unsigned long long> &budget_yields_ref() // budget waits of this process that ran out of patience (diagnostics)
{
    static std::atomic<unsigned long long> n{0};
    return n;
}

// a HIP stream with shared ownership: buffers remember the streams that touched them, so a stream outlives its block while a message
// that names it is still in flight
struct StreamRef {
    void *s = nullptr;
    StreamRef() { check(api().stream_create(&s)); }
    ~StreamRef()
    {
        api().stream_sync(s); // a block that ends (hang-up) lets its queued work finish before the stream goes
        api().stream_destroy(s);
    }
    StreamRef(const StreamRef &) = delete;
    StreamRef &operator=(const StreamRef &) = delete;
};
enum StreamPolicy { SHARED = 0, PER_BLOCK = 1 };
inline std::atomic<int> &stream_policy_ref()
{
    static std::atomic<int> p{SHARED};
    return p;
}
inline void set_stream_policy(StreamPolicy p) { stream_policy_ref().store(p); }
// the one compute stream of the calling thread's current device, created on first use, kept for the life of the process
inline std::shared_ptr<StreamRef> graph_stream()
{
    static std::mutex m;
    static std::map<int, std::shared_ptr<StreamRef>> *streams = new std::map<int, std::shared_ptr<StreamRef>>(); // never destroyed: no HIP calls at exit
    int d = 0;
    check(api().get_device(&d));
    std::lock_guard<std::mutex> l(m);
    auto &p = (*streams)[d];
    if (!p) p = std::make_shared<StreamRef>();
    return p;
}

// Every block runs on its own OS thread (src/ratpak.rs:60-185) and enqueues on the stream it holds for its life: COMPUTE blocks on
// the device's shared graph stream (PER_BLOCK policy: one of their own), TRANSFER blocks always on one of their own.
struct BlockStream {
    enum Kind { COMPUTE, TRANSFER };
    std::shared_ptr<StreamRef> ref;
    explicit BlockStream(Kind k = COMPUTE)
        : ref(k == COMPUTE && stream_policy_ref().load() == SHARED ? graph_stream() : std::make_shared<StreamRef>()) {}
    BlockStream(const BlockStream &) = delete;
    BlockStream &operator=(const BlockStream &) = delete;
    operator void *() const { return ref->s; }
};

// one device buffer and what orders its uses: the stream that wrote it last, the streams that have read it since
struct Buf {
    void *ptr = nullptr;
    size_t cap = 0;
    std::mutex m; // the readers of a forked message register from several threads
    std::shared_ptr<StreamRef> writer;
    std::vector<std::shared_ptr<StreamRef>> readers;
    void *event = nullptr; // used under m for a record-there / wait-here pair; may be re-recorded as soon as the wait has been enqueued
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    int grow(size_t bytes)
    {
        if (ptr) api().free_(ptr);
        ptr = nullptr; cap = 0;
        int rc = api().malloc_(&ptr, bytes ? bytes : 1);
        if (rc == REDIO_OK) cap = bytes;
        return rc;
    }
    ~Buf()
    {
        if (ptr) api().free_(ptr);
        if (event) api().event_destroy(event);
    }
    // work enqueued on `mine` from now on runs after everything `other` holds at this moment (m held)
    void order_after(const std::shared_ptr<StreamRef> &other, void *mine)
    {
        if (!other || other->s == mine) return; // same queue: already ordered
        if (!event) check(api().event_create(&event));
        check(api().event_record(event, other->s));
        check(api().stream_wait_event(mine, event));
    }
    void wait_writer(void *mine)
    {
        std::lock_guard<std::mutex> l(m);
        order_after(writer, mine);
    }
    void add_reader(const std::shared_ptr<StreamRef> &st)
    {
        std::lock_guard<std::mutex> l(m);
        for (auto &r : readers) if (r->s == st->s) return;
        readers.push_back(st);
    }
    // ring recycling (nobody else holds the buffer): the new writer's stream waits for the previous message's readers and writer
    void begin_write(void *mine)
    {
        std::lock_guard<std::mutex> l(m);
        for (auto &r : readers) order_after(r, mine);
        if (readers.empty()) order_after(writer, mine);
        readers.clear();
        writer.reset();
    }
    void end_write(const std::shared_ptr<StreamRef> &st)
    {
        std::lock_guard<std::mutex> l(m);
        writer = st;
    }
};

namespace detail {
struct RingState {
    std::mutex m;
    std::condition_variable cv;
    std::vector<std::unique_ptr<Buf>> free; // buffers nobody holds
    size_t depth = 0, live = 0;             // live: buffers that exist (free + leased)
    size_t budget = (size_t)-1, out = 0, out_bytes = 0; // leased buffers and the message bytes in them, against the byte budget
    bool closed = false;
    unsigned long long yields = 0;          // times the byte budget gave way
    int impatient = 0;                      // ... in a row
    unsigned long long grows = 0;           // device allocations this ring made (warm-up, or a message larger than any before)
};
// size classes: the request rounded up to 1/8 of its leading power of two (<= 12.5 % slack), so that messages whose length wobbles
// (the resampler's floor(ratio * len + 1)) keep hitting the same buffers
inline size_t size_class(size_t bytes)
{
    if (bytes <= 256) return 256;
    size_t p = 1;
    while ((p << 1) <= bytes) p <<= 1;
    const size_t q = p >> 3;
    return (bytes + q - 1) / q * q;
}
} // namespace detail

// the lease of one buffer: a message's storage.  Dropping the last handle returns the buffer to its ring (or frees a standalone one).
struct Alloc {
    void *ptr = nullptr;
    size_t bytes = 0;
    std::unique_ptr<Buf> buf;
    std::shared_ptr<detail::RingState> home;
    Alloc() = default;
    // standalone buffer (constants, test fixtures, the unpooled mode): freed when the last handle drops -- hipFree, a device-wide wait
    explicit Alloc(size_t b) : bytes(b), buf(new Buf)
    {
        check(buf->grow(b ? b : 1));
        ptr = buf->ptr;
    }
    Alloc(const Alloc &) = delete;
    Alloc &operator=(const Alloc &) = delete;
    ~Alloc()
    {
        if (!home || !buf) return; // standalone: ~Buf frees
        {
            std::lock_guard<std::mutex> l(home->m);
            --home->out;
            home->out_bytes -= bytes;
            if (home->closed) { --home->live; return; } // the block is gone: ~Buf frees
            home->free.push_back(std::move(buf));
        }
        home->cv.notify_all();
    }
};

template <typename T>
struct View {
    std::shared_ptr<Alloc> mem;
    size_t off = 0, len = 0; // in elements of T
    T *data() const { return reinterpret_cast<T *>(mem->ptr) + off; }
    View sub(size_t o, size_t n) const { return View{mem, off + o, n}; }
};

// scope of a block's reads of one input message on its stream: orders the stream behind the message's writer at entry, registers the
// stream as a reader at exit (the buffer is not rewritten before what this stream holds then).  complete(): the reads are known to
// have finished (the block synchronised with the host), nothing to register.
template <typename T>
struct Reading {
    const View<T> &v;
    const BlockStream &st;
    bool finished = false;
    Reading(const View<T> &view, const BlockStream &stream) : v(view), st(stream)
    {
        if (v.mem && v.mem->buf) v.mem->buf->wait_writer(st);
    }
    void complete() { finished = true; }
    ~Reading()
    {
        if (!finished && v.mem && v.mem->buf) v.mem->buf->add_reader(st.ref);
    }
    Reading(const Reading &) = delete;
    Reading &operator=(const Reading &) = delete;
};

// standalone message (not pooled): constants, fixtures
template <typename T>
View<T> make(size_t n) { return View<T>{std::make_shared<Alloc>(n * sizeof(T)), 0, n}; }

// the per-block ring of output buffers (header comment).  depth 0: every acquire allocates (unpooled).
class Ring {
    std::shared_ptr<detail::RingState> s_;
    bool first_fill_ = true; // acquire() is called by the ring's own block thread only

public:
    explicit Ring(size_t depth = default_ring_depth_ref().load(), size_t byte_budget = default_ring_bytes_ref().load())
        : s_(std::make_shared<detail::RingState>())
    {
        s_->depth = depth;
        s_->budget = byte_budget;
    }
    Ring(const Ring &) = delete;
    Ring &operator=(const Ring &) = delete;
    ~Ring()
    {
        std::vector<std::unique_ptr<Buf>> drop;
        {
            std::lock_guard<std::mutex> l(s_->m);
            s_->closed = true;
            s_->live -= s_->free.size();
            drop.swap(s_->free);
        }
        s_->cv.notify_all();
    } // buffers still held downstream are freed by their last handle
    size_t depth() const { return s_->depth; }
    unsigned long long budget_yields() const
    {
        std::lock_guard<std::mutex> l(s_->m);
        return s_->yields;
    }
    unsigned long long grows() const
    {
        std::lock_guard<std::mutex> l(s_->m);
        return s_->grows;
    }
    // a buffer of n elements for work to be enqueued on `stream`; waits for a credit while all `depth` buffers, or the byte budget's
    // worth of messages, are held downstream
    template <typename T>
    View<T> acquire(size_t n, void *stream)
    {
        const size_t bytes = n * sizeof(T);
        if (s_->depth == 0) return make<T>(n);
        std::unique_ptr<Buf> b;
        {
            std::unique_lock<std::mutex> l(s_->m);
            // a message larger than the cache (twice the budget) cannot be kept there whatever the order: holding its producer back gains
            // nothing; one between the budget and the cache goes alone
            const bool too_big = s_->budget != (size_t)-1 && bytes / 2 > s_->budget;
            const auto in_budget = [&] { return s_->out == 0 || (s_->out < s_->depth && (too_big || s_->out_bytes + bytes <= s_->budget)); };
            while (!in_budget()) {
                if (s_->out >= s_->depth) s_->cv.wait(l); // no credit: the bound
                // (wait_until on the system clock = pthread_cond_timedwait, which ThreadSanitizer follows; wait_for goes through
                // pthread_cond_clockwait, which gcc 11's does not: it then believes the waiter still holds the mutex)
                else if (s_->cv.wait_until(l, std::chrono::system_clock::now() + std::chrono::milliseconds(ring_patience_ms_ref().load()), in_budget))
                    s_->impatient = 0;
                else { // comment at ring_patience_ms_ref: this message goes now (out < depth); three in a row and the budget is off
                    ++s_->yields;
                    ++budget_yields_ref();
                    if (++s_->impatient >= 3) s_->budget = (size_t)-1;
                    break;
                }
            }
            // best fit among the free buffers, the one released last among equals (the likeliest to be in the cache still); else a new
            // one while the ring is not full; else the largest free one is regrown
            size_t best = s_->free.size();
            for (size_t i = 0; i < s_->free.size(); ++i)
                if (s_->free[i]->cap >= bytes && (best == s_->free.size() || s_->free[i]->cap <= s_->free[best]->cap)) best = i;
            if (best == s_->free.size() && s_->live >= s_->depth) {
                best = 0;
                for (size_t i = 1; i < s_->free.size(); ++i) if (s_->free[i]->cap > s_->free[best]->cap) best = i;
            }
            if (best < s_->free.size()) {
                b = std::move(s_->free[best]);
                s_->free.erase(s_->free.begin() + (long)best);
            } else {
                b.reset(new Buf);
                ++s_->live;
            }
            if (b->cap < bytes || !b->ptr) ++s_->grows;
            ++s_->out;
            s_->out_bytes += bytes;
        }
        if (b->cap < bytes || !b->ptr) {
            // rare: warm-up, or the largest message so far (hipFree + hipMalloc).  One eighth of headroom on top of the size class: a block whose
            // messages wobble across a class boundary (the stream blocks send 12 or 13 spectra per 2^16-sample message) then settles at once
            const int rc = b->grow(detail::size_class(bytes + bytes / 8));
            if (rc != REDIO_OK) {
                { std::lock_guard<std::mutex> l(s_->m); --s_->live; --s_->out; s_->out_bytes -= bytes; }
                s_->cv.notify_all();
                check(rc);
            }
        }
        if (first_fill_) { // the ring's first message: the other buffers of its size class now, so that a graph allocates during its
            first_fill_ = false; // first message and never after (a fourth buffer first needed deep into a run would be a late hipMalloc).
            // As many as the byte budget lets out at this message size, and one to spare for lengths that wobble
            const size_t want = bytes / 2 > s_->budget ? s_->depth : std::min(s_->depth, s_->budget / std::max<size_t>(bytes, 1) + 1 + (bytes > s_->budget));
            for (size_t i = 1; i < want; ++i) {
                std::unique_ptr<Buf> extra(new Buf);
                if (extra->grow(b->cap) != REDIO_OK) break; // the ring then holds fewer buffers until a later acquire can allocate
                std::lock_guard<std::mutex> l(s_->m);
                ++s_->live; ++s_->grows;
                s_->free.push_back(std::move(extra));
            }
        }
        auto a = std::make_shared<Alloc>();
        a->ptr = b->ptr;
        a->bytes = bytes;
        a->buf = std::move(b);
        a->home = s_;
        a->buf->begin_write(stream); // the previous message's readers finish before this stream writes
        return View<T>{std::move(a), 0, n};
    }
};

// producer side of every block: the work that fills the message has been enqueued on the block's stream (in the debugging mode: and
// has finished)
template <typename T>
void publish(const View<T> &o, const BlockStream &st)
{
    if (host_sync_flag().load(std::memory_order_relaxed)) {
        check(redio_stream_sync(st));
        o.mem->buf->end_write(nullptr); // complete: nobody needs to wait
    } else o.mem->buf->end_write(st.ref);
}

// host Vec<T> -> device View<T> and back (the only PCIe crossings of a device-resident graph)
template <typename T>
void to_device(Receiver<std::vector<T>> u, Sender<View<T>> v)
{
    BlockStream st(BlockStream::TRANSFER);
    Ring ring(default_ring_depth_ref().load(), (size_t)-1); // no byte budget: the copy engine fills the next message while the graph works on this one
    for (;;) {
        auto x = u.recv();
        auto d = ring.acquire<T>(x.size(), st);
        check(redio_upload(d.data(), x.data(), x.size() * sizeof(T), st));
        check(redio_stream_sync(st)); // the pageable source Vec is freed when this iteration ends
        d.mem->buf->end_write(nullptr); // the copy has finished: consumers have nothing to wait for
        v.send_unwrap(std::move(d));
    }
}
template <typename T>
void to_host(Receiver<View<T>> u, Sender<std::vector<T>> v)
{
    BlockStream st(BlockStream::TRANSFER);
    for (;;) {
        auto d = u.recv();
        std::vector<T> x(d.len);
        {
            Reading<T> in(d, st);
            check(redio_download(x.data(), d.data(), d.len * sizeof(T), st));
            check(redio_stream_sync(st)); // data handed to the CPU: the one place a graph waits on the host
            in.complete();
        }
        v.send_unwrap(std::move(x));
    }
}

// test / bench source: nmsg messages of msg_len hash-generated cf32 samples, message i = samples [i*msg_len, (i+1)*msg_len)
inline void synth_iq_source(Sender<View<std::complex<float>>> v, uint32_t seed, size_t msg_len, size_t nmsg)
{
    BlockStream st;
    Ring ring;
    for (size_t i = 0; i < nmsg; ++i) {
        auto d = ring.acquire<std::complex<float>>(msg_len, st);
        check(redio_synth_iq(d.data(), seed, (uint64_t)i * msg_len, msg_len, st));
        publish(d, st);
        v.send_unwrap(std::move(d));
    }
}

// checking sink: the order-free sum of every 32-bit word received (redio_checksum_u32) and the message count, written at hang-up
template <typename T>
void checksum_sink(Receiver<View<T>> u, unsigned long long *sum, size_t *messages)
{
    BlockStream st;
    auto acc = make<unsigned long long>(1);
    const unsigned long long zero = 0;
    check(redio_upload(acc.data(), &zero, sizeof(zero), st));
    check(redio_stream_sync(st));
    size_t n = 0;
    try {
        for (;;) {
            auto d = u.recv();
            Reading<T> in(d, st);
            check(redio_checksum_u32(d.data(), d.len * sizeof(T) / 4, acc.data(), st));
            ++n;
        }
    } catch (const hangup &) {
    }
    unsigned long long s = 0;
    check(redio_download(&s, acc.data(), sizeof(s), st));
    check(redio_stream_sync(st));
    if (sum) *sum = s;
    if (messages) *messages = n;
}

// kpn::shaper on a View stream: chunks of exactly l samples; zero-copy when possible, otherwise the
// straddling chunk is assembled once on the device.  A trailing partial chunk is dropped at hang-up.
template <typename T>
void shaper(Receiver<View<T>> u, Sender<View<T>> v, size_t l)
{
    BlockStream st;
    Ring ring;
    View<T> pend;           // partially filled chunk (owned copy)
    size_t have = 0;
    for (;;) {
        auto d = u.recv();
        size_t pos = 0;
        while (pos < d.len) {
            if (have == 0 && d.len - pos >= l) { // whole chunk inside this message: a view (the producer's events travel with it)
                v.send_unwrap(d.sub(pos, l));
                pos += l;
                continue;
            }
            if (have == 0) pend = ring.acquire<T>(l, st);
            const size_t take = std::min(l - have, d.len - pos);
            {
                Reading<T> in(d, st);
                check(redio_copy(pend.data() + have, d.data() + pos, take * sizeof(T), st));
            }
            have += take;
            pos += take;
            if (have == l) {
                publish(pend, st);
                v.send_unwrap(std::move(pend));
                pend = View<T>();
                have = 0;
            }
        }
    }
}

namespace detail {
// the loop every stateless hot block shares: recv -> ring buffer of nout(d) samples -> enqueue on the block's stream between the
// input's `ready` wait and its `done` record -> `ready` of the output -> send
template <typename In, typename Out, typename NOut, typename Enqueue>
void run_block(Receiver<View<In>> &u, Sender<View<Out>> &v, NOut nout, Enqueue enqueue)
{
    BlockStream st;
    Ring ring;
    for (;;) {
        auto d = u.recv();
        auto o = ring.acquire<Out>(nout(d), st);
        {
            Reading<In> in(d, st);
            check(enqueue(d, o, (void *)st));
        }
        publish(o, st);
        v.send_unwrap(std::move(o));
    }
}

// run_block with coalescing (coalesce_limit_ref): recv, then whatever try_recv() finds queued, up to `limit` messages and about
// COALESCE_MAX_IN input elements; one ring buffer for the batch's outputs (each at a 256-byte aligned offset); one Reading scope per
// input around the ONE enqueue_list(inputs, buffer, offsets, stream) call; publish; the outputs sent in order as views of the buffer.
// A hang-up while a batch is open ends the block only after that batch has gone out (try_recv never throws; the next recv() does).
template <typename In, typename Out, typename NOut, typename EnqueueList>
void run_block_list(Receiver<View<In>> &u, Sender<View<Out>> &v, NOut nout, EnqueueList enqueue_list, size_t limit = coalesce_limit_ref().load())
{
    static_assert(256 % sizeof(Out) == 0, "outputs at 256-byte offsets");
    constexpr size_t ALIGN = 256 / sizeof(Out);
    BlockStream st;
    Ring ring;
    std::vector<View<In>> ins;
    std::vector<size_t> offs, lens;
    size_t high = 0; // the largest batch buffer so far: every buffer of the ring settles at it, so batches of varying sizes stop regrowing them
    for (;;) {
        ins.clear();
        ins.push_back(u.recv());
        size_t in_elems = ins[0].len;
        while (ins.size() < limit && in_elems < COALESCE_MAX_IN) {
            auto d = u.try_recv();
            if (!d) break;
            in_elems += d->len;
            ins.push_back(std::move(*d));
        }
        offs.resize(ins.size());
        lens.resize(ins.size());
        size_t total = 0;
        for (size_t i = 0; i < ins.size(); ++i) {
            offs[i] = (total + ALIGN - 1) / ALIGN * ALIGN;
            lens[i] = nout(ins[i]);
            total = offs[i] + lens[i];
        }
        high = std::max(high, total);
        auto o = ring.acquire<Out>(high, st);
        {
            std::vector<std::unique_ptr<Reading<In>>> rd;
            for (auto &d : ins) rd.emplace_back(new Reading<In>(d, st));
            check(enqueue_list(ins, o, offs, (void *)st));
        }
        publish(o, st);
        for (size_t i = 0; i < ins.size(); ++i) v.send_unwrap(o.sub(offs[i], lens[i]));
    }
}
} // namespace detail

// dsputils::convolve semantics on device streams (complex samples x real taps, optional decimation)
inline void fir(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps, size_t decim, bool fused)
{
    using cf = std::complex<float>;
    redio_fir *h = nullptr;
    check(redio_fir_create(&h, taps.data(), taps.size(), decim, REDIO_FIR_COMPLEX | (fused ? REDIO_FIR_FUSED : 0)));
    struct G { redio_fir *h; ~G() { redio_fir_destroy(h); } } g{h};
    detail::run_block<cf, cf>(u, v, [&](const View<cf> &d) { return redio_fir_nout(h, d.len); },
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_fir_enqueue(h, d.data(), d.len, o.data(), st); });
}

// kissfft::fft semantics: every message must be a whole number of block_size-sample blocks
inline void fft(Receiver<View<std::complex<float>>> pin, Sender<View<std::complex<float>>> cout, uint32_t block_size, uint32_t inv)
{
    using cf = std::complex<float>;
    redio_fft *h = nullptr;
    check(redio_fft_create(&h, (int)block_size, (int)inv));
    struct G { redio_fft *h; ~G() { redio_fft_destroy(h); } } g{h};
    const auto nout = [&](const View<cf> &d) {
        if (d.len % block_size) throw std::runtime_error("assert!(din.len() == block_size) (kissfft.rs:24)");
        return d.len;
    };
    if (coalesce_limit_ref().load() > 1) { // several queued messages in one launch (coalesce_limit_ref)
        detail::run_block_list<cf, cf>(pin, cout, nout, [&](const std::vector<View<cf>> &ds, const View<cf> &o, const std::vector<size_t> &offs, void *st) {
            std::vector<redio_msg> m(ds.size());
            for (size_t i = 0; i < ds.size(); ++i) m[i] = redio_msg{ds[i].data(), ds[i].len / block_size, o.data() + offs[i]};
            return redio_fft_enqueue_list(h, m.data(), m.size(), st);
        });
        return;
    }
    detail::run_block<cf, cf>(pin, cout, nout,
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_fft_enqueue(h, d.data(), o.data(), d.len / block_size, st); });
}

// kiss_fftr as a block (redio_fftr_*): every message is a whole number of block_size real samples; each block of block_size
// samples becomes block_size / 2 + 1 bins.  Output through the ring, no host wait.
inline void fftr(Receiver<View<float>> pin, Sender<View<std::complex<float>>> cout, uint32_t block_size)
{
    using cf = std::complex<float>;
    redio_fftr *h = nullptr;
    check(redio_fftr_create(&h, (int)block_size, 0));
    struct G { redio_fftr *h; ~G() { redio_fftr_destroy(h); } } g{h};
    const size_t nbins = block_size / 2 + 1;
    detail::run_block<float, cf>(pin, cout,
                                 [&](const View<float> &d) {
                                     if (d.len % block_size) throw std::runtime_error("assert!(din.len() == block_size) (kissfft.rs:24)");
                                     return d.len / block_size * nbins;
                                 },
                                 [&](const View<float> &d, const View<cf> &o, void *st) { return redio_fftr_enqueue(h, d.data(), o.data(), d.len / block_size, st); });
}

// kiss_fftri as a block: every message is a whole number of block_size / 2 + 1 bins; each becomes block_size real samples (unnormalised)
inline void fftri(Receiver<View<std::complex<float>>> pin, Sender<View<float>> cout, uint32_t block_size)
{
    using cf = std::complex<float>;
    redio_fftr *h = nullptr;
    check(redio_fftr_create(&h, (int)block_size, 1));
    struct G { redio_fftr *h; ~G() { redio_fftr_destroy(h); } } g{h};
    const size_t nbins = block_size / 2 + 1;
    detail::run_block<cf, float>(pin, cout,
                                 [&](const View<cf> &d) {
                                     if (d.len % nbins) throw std::runtime_error("assert!(din.len() == block_size) (kissfft.rs:24)");
                                     return d.len / nbins * (size_t)block_size;
                                 },
                                 [&](const View<cf> &d, const View<float> &o, void *st) { return redio_fftr_enqueue(h, d.data(), o.data(), d.len / nbins, st); });
}

// the fused north-star chain as one block
inline void fir_fft_chain(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps,
                          size_t decim, int nfft, bool fused)
{
    using cf = std::complex<float>;
    redio_chain *h = nullptr;
    check(redio_chain_create(&h, taps.data(), taps.size(), decim, nfft, fused ? REDIO_FIR_FUSED : 0));
    struct G { redio_chain *h; ~G() { redio_chain_destroy(h); } } g{h};
    const auto nout = [&](const View<cf> &d) { return redio_chain_nblocks(h, d.len) * (size_t)nfft; };
    if (coalesce_limit_ref().load() > 1) { // several queued messages in one launch (coalesce_limit_ref)
        detail::run_block_list<cf, cf>(u, v, nout, [&](const std::vector<View<cf>> &ds, const View<cf> &o, const std::vector<size_t> &offs, void *st) {
            std::vector<redio_msg> m(ds.size());
            for (size_t i = 0; i < ds.size(); ++i) m[i] = redio_msg{ds[i].data(), ds[i].len, o.data() + offs[i]};
            return redio_chain_enqueue_list(h, m.data(), m.size(), st);
        });
        return;
    }
    detail::run_block<cf, cf>(u, v, nout,
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_chain_enqueue(h, d.data(), d.len, o.data(), st); });
}

// the receiver's messages straight into the chain: u8 I/Q bytes (rtlsdr::rtlSource, rtlsdr.rs:127-152) -> data_to_samples
// (rtlsdr.rs:159-162) -> FIR -> FFT as ONE kernel for the north-star shape (redio_chain_enqueue_u8)
inline void bytes_fir_fft_chain(Receiver<View<uint8_t>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps, size_t decim, int nfft,
                                bool fused)
{
    using cf = std::complex<float>;
    redio_chain *h = nullptr;
    check(redio_chain_create(&h, taps.data(), taps.size(), decim, nfft, fused ? REDIO_FIR_FUSED : 0));
    struct G { redio_chain *h; ~G() { redio_chain_destroy(h); } } g{h};
    detail::run_block<uint8_t, cf>(u, v, [&](const View<uint8_t> &d) { return redio_chain_nblocks(h, d.len / 2) * (size_t)nfft; },
                                   [&](const View<uint8_t> &d, const View<cf> &o, void *st) { return redio_chain_enqueue_u8(h, d.data(), d.len, o.data(), st); });
}

// the front end of the shipped graph: u8 IQ bytes -> |x| (rtlsdr.rs:159-162 + ratpak.rs:64-68)
inline void ingest_mag(Receiver<View<uint8_t>> u, Sender<View<float>> v)
{
    detail::run_block<uint8_t, float>(u, v, [](const View<uint8_t> &d) { return d.len / 2; },
                                      [](const View<uint8_t> &d, const View<float> &o, void *st) { return redio_ingest_u8_mag(d.data(), d.len, o.data(), st); });
}

// kpn::mul_vecs / sum_vecs (kpn.rs:198-203, 227-231) with the constant vector resident on the device
namespace detail {
inline int zip_call(bool add, const float *a, const float *b, float *o, size_t n, void *st) { return add ? redio_add_f32(a, b, o, n, st) : redio_mul_f32(a, b, o, n, st); }
inline int zip_call(bool add, const std::complex<float> *a, const std::complex<float> *b, std::complex<float> *o, size_t n, void *st)
{
    return add ? redio_add_c32(a, b, o, n, st) : redio_mul_c32(a, b, o, n, st);
}
template <typename T>
void zip_vecs(Receiver<View<T>> u, Sender<View<T>> v, const std::vector<T> &c, bool add)
{
    auto dc = make<T>(c.size());
    check(redio_upload(dc.data(), c.data(), c.size() * sizeof(T), nullptr));
    check(redio_stream_sync(nullptr)); // once, before the first message: the constant is resident from here on
    run_block<T, T>(u, v, [&](const View<T> &x) { return x.len < c.size() ? x.len : c.size(); },
                    [&](const View<T> &x, const View<T> &o, void *st) { return zip_call(add, x.data(), dc.data(), o.data(), o.len, st); });
}
} // namespace detail
template <typename T>
void mul_vecs(Receiver<View<T>> u, Sender<View<T>> v, std::vector<T> c) { detail::zip_vecs<T>(std::move(u), std::move(v), c, false); }
template <typename T>
void sum_vecs(Receiver<View<T>> u, Sender<View<T>> v, std::vector<T> c) { detail::zip_vecs<T>(std::move(u), std::move(v), c, true); }

// samplerate::resample semantics (samplerate.rs:59-87) on a device stream: one converter state for the
// life of the block, output capacity floor(ratio*len + 1) per message, output_frames_gen samples sent
inline void resample(Receiver<View<float>> din, Sender<View<float>> dout, double ratio)
{
    BlockStream st(BlockStream::TRANSFER); // redio_src_process synchronises its stream (host state machine): keep that off the graph stream
    Ring ring;
    redio_src *h = nullptr;
    int rc = redio_src_create(&h, 1 /* SRC_SINC_MEDIUM_QUALITY, samplerate.rs:27 */, 1);
    if (rc != REDIO_OK) throw std::runtime_error(redio_strerror(rc));
    struct G { redio_src *h; ~G() { redio_src_destroy(h); } } g{h};
    for (;;) {
        auto d = din.recv();
        const long lout = (long)(ratio * (double)d.len + 1.0);
        auto o = ring.acquire<float>((size_t)lout, st);
        long used = 0, gen = 0;
        {
            Reading<float> in(d, st);
            // synchronises the stream itself: the converter's per-output parameters come from its host state machine
            rc = redio_src_process(h, d.data(), (long)d.len, (long)d.len, o.data(), lout, lout, ratio, 0, &used, &gen, st);
            if (rc == REDIO_OK) in.complete();
        }
        if (rc != REDIO_OK) throw std::runtime_error(redio_strerror(rc)); // the reference panics with src_strerror's text
        o.mem->buf->end_write(nullptr); // finished (synchronised above)
        dout.send_unwrap(o.sub(0, (size_t)gen));
    }
}

// nch mono streams through ONE batched converter in stream order (redio_src_enqueue): a message is [nch][frames] flattened, every
// row one stream with samplerate::resample's semantics (output capacity floor(ratio*frames + 1) per row, samplerate.rs:59-87); the
// message sent is [nch][gen] packed.  A compute block on the graph stream: after the first message at a constant ratio with integer
// 1/ratio nothing synchronises (redio_src_enqueue_counts), the input is released by stream order like every other block's.  When
// `counts` is given the handle's (queued, synchronised) call counts are written there at hang-up (tests, tools).
inline void resample_channels(Receiver<View<float>> din, Sender<View<float>> dout, int nch, double ratio, int converter = 1,
                              int mode = REDIO_SRC_EXACT, long *counts = nullptr)
{
    if (nch < 1) throw std::runtime_error("resample_channels: nch < 1");
    BlockStream st;
    Ring ring;
    redio_src *h = nullptr;
    check(redio_src_create(&h, converter, nch));
    struct G {
        redio_src *h; long *counts;
        ~G()
        {
            if (counts) redio_src_enqueue_counts(h, counts, counts + 1);
            redio_src_destroy(h);
        }
    } g{h, counts};
    check(redio_src_set_mode(h, mode));
    for (;;) {
        auto d = din.recv();
        if (d.len % (size_t)nch) throw std::runtime_error("resample_channels: message length is not a multiple of the channel count");
        const long frames = (long)(d.len / (size_t)nch);
        const long lout = (long)(ratio * (double)frames + 1.0);
        auto o = ring.acquire<float>((size_t)lout * (size_t)nch, st);
        long used = 0, gen = 0;
        {
            Reading<float> in(d, st);
            check(redio_src_enqueue(h, d.data(), frames, frames, o.data(), lout, 0 /* packed */, ratio, &used, &gen, st));
        }
        publish(o, st);
        dout.send_unwrap(o.sub(0, (size_t)gen * (size_t)nch));
    }
}

// the channelizer's rows [nrows][nchan] cf32 -> [2*nchan][nrows] f32, plane 2c = Re and 2c + 1 = Im of channel c: resample_channels'
// message for 2*nchan streams; and back
inline void channel_planes(Receiver<View<std::complex<float>>> u, Sender<View<float>> v, int nchan)
{
    using cf = std::complex<float>;
    if (nchan < 1) throw std::runtime_error("channel_planes: nchan < 1");
    detail::run_block<cf, float>(u, v,
                                 [&](const View<cf> &d) {
                                     if (d.len % (size_t)nchan) throw std::runtime_error("channel_planes: message is not whole rows");
                                     return 2 * d.len;
                                 },
                                 [&](const View<cf> &d, const View<float> &o, void *st) {
                                     const size_t nrows = d.len / (size_t)nchan;
                                     return redio_rows_to_planes_c32(d.data(), nrows, nchan, o.data(), nrows, st);
                                 });
}
inline void plane_rows(Receiver<View<float>> u, Sender<View<std::complex<float>>> v, int nchan)
{
    using cf = std::complex<float>;
    if (nchan < 1) throw std::runtime_error("plane_rows: nchan < 1");
    detail::run_block<float, cf>(u, v,
                                 [&](const View<float> &d) {
                                     if (d.len % (2 * (size_t)nchan)) throw std::runtime_error("plane_rows: message is not whole planes");
                                     return d.len / 2;
                                 },
                                 [&](const View<float> &d, const View<cf> &o, void *st) {
                                     const size_t nrows = d.len / (2 * (size_t)nchan);
                                     return redio_planes_to_rows_c32(d.data(), nrows, nrows, nchan, o.data(), st);
                                 });
}

// the 64-channel polyphase filterbank (BASELINE configs[3]) as a block: rows of 64 channel samples out
inline void channelizer(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                        int taps_per_branch, bool fused)
{
    using cf = std::complex<float>;
    redio_pfb *h = nullptr;
    check(redio_pfb_create(&h, proto.data(), nchan, taps_per_branch, fused ? REDIO_FIR_FUSED : 0));
    struct G { redio_pfb *h; ~G() { redio_pfb_destroy(h); } } g{h};
    detail::run_block<cf, cf>(u, v, [&](const View<cf> &d) { return redio_pfb_nrows(h, d.len) * (size_t)nchan; },
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_pfb_enqueue(h, d.data(), d.len, o.data(), 1, st); });
}

// overlap-save FFT convolution (BASELINE configs[4]) with dsputils::convolve's valid-mode semantics per message
inline void overlap_save(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps, int nfft)
{
    using cf = std::complex<float>;
    redio_ovsave *h = nullptr;
    check(redio_ovsave_create(&h, taps.data(), taps.size(), nfft));
    struct G { redio_ovsave *h; ~G() { redio_ovsave_destroy(h); } } g{h};
    detail::run_block<cf, cf>(u, v, [&](const View<cf> &d) { return redio_ovsave_nout(h, d.len); },
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_ovsave_enqueue(h, d.data(), d.len, o.data(), st); });
}

// ---- the windowed blocks as STREAMS: history carried across messages on the device (redio_*_stream_*, include/redio.h) ----
// The blocks above keep the reference's per-message semantics (dsputils::convolve is stateless, dsputils.rs:30-32: a
// message seam costs ntaps - 1 outputs).  These carry the stream's unconsumed tail in HBM, so the concatenation of their
// output messages does not depend on how the input was cut into messages; a message that completes no
// output unit sends nothing.  The seam is staged by work on the block's own stream, inside the input's Reading scope, so the
// input buffer may be recycled as soon as that scope's `done` event has passed.
namespace detail {
template <typename TI, typename TO, typename NOut, typename Enqueue>
void run_stream_block_of(Receiver<View<TI>> &u, Sender<View<TO>> &v, NOut nout, Enqueue enqueue)
{
    BlockStream st;
    Ring ring;
    for (;;) {
        auto d = u.recv();
        const size_t n = nout(d.len);
        auto o = n ? ring.acquire<TO>(n, st) : View<TO>();
        size_t got = 0;
        {
            Reading<TI> in(d, st);
            check(enqueue(d, n ? o.data() : nullptr, &got, (void *)st));
        }
        if (n) {
            publish(o, st);
            v.send_unwrap(std::move(o));
        }
    }
}
template <typename NOut, typename Enqueue>
void run_stream_block(Receiver<View<std::complex<float>>> &u, Sender<View<std::complex<float>>> &v, NOut nout, Enqueue enqueue)
{
    run_stream_block_of<std::complex<float>, std::complex<float>>(u, v, nout, enqueue);
}
} // namespace detail

inline void fir_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps, size_t decim, bool fused)
{
    using cf = std::complex<float>;
    redio_fir *h = nullptr;
    check(redio_fir_create(&h, taps.data(), taps.size(), decim, REDIO_FIR_COMPLEX | (fused ? REDIO_FIR_FUSED : 0)));
    redio_fir_stream *s = nullptr;
    const int rc = redio_fir_stream_create(&s, h);
    struct G { redio_fir *h; redio_fir_stream *s; ~G() { redio_fir_stream_destroy(s); redio_fir_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_fir_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_fir_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

inline void fir_fft_chain_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps,
                                 size_t decim, int nfft, bool fused)
{
    using cf = std::complex<float>;
    redio_chain *h = nullptr;
    check(redio_chain_create(&h, taps.data(), taps.size(), decim, nfft, fused ? REDIO_FIR_FUSED : 0));
    redio_chain_stream *s = nullptr;
    const int rc = redio_chain_stream_create(&s, h);
    struct G { redio_chain *h; redio_chain_stream *s; ~G() { redio_chain_stream_destroy(s); redio_chain_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_chain_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_chain_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

inline void channelizer_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                               int taps_per_branch, bool fused)
{
    using cf = std::complex<float>;
    redio_pfb *h = nullptr;
    check(redio_pfb_create(&h, proto.data(), nchan, taps_per_branch, fused ? REDIO_FIR_FUSED : 0));
    redio_pfb_stream *s = nullptr;
    const int rc = redio_pfb_stream_create(&s, h);
    struct G { redio_pfb *h; redio_pfb_stream *s; ~G() { redio_pfb_stream_destroy(s); redio_pfb_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_pfb_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_pfb_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

// the synthesis filterbank (redio_pfb_synth_*: the inverse transform of every row of nchan channel values, then the channelizer's
// branch filter) as a block: rows of channel values in -- dev::channelizer's output -- samples of ONE stream out.
// Per message: the first taps_per_branch - 1 rows of a message only fill the filter.
inline void synthesizer(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                        int taps_per_branch, bool fused)
{
    using cf = std::complex<float>;
    redio_pfb_synth *h = nullptr;
    check(redio_pfb_synth_create(&h, proto.data(), nchan, taps_per_branch, fused ? REDIO_FIR_FUSED : 0));
    struct G { redio_pfb_synth *h; ~G() { redio_pfb_synth_destroy(h); } } g{h};
    detail::run_block<cf, cf>(u, v, [&](const View<cf> &d) { return redio_pfb_synth_nout(h, d.len); },
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_pfb_synth_enqueue(h, d.data(), d.len, o.data(), st); });
}

// ... and as a stream: messages of any length, taps_per_branch - 1 rows and a partial row carried, whole output rows sent
inline void synthesizer_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                               int taps_per_branch, bool fused)
{
    using cf = std::complex<float>;
    redio_pfb_synth *h = nullptr;
    check(redio_pfb_synth_create(&h, proto.data(), nchan, taps_per_branch, fused ? REDIO_FIR_FUSED : 0));
    redio_pfb_synth_stream *s = nullptr;
    const int rc = redio_pfb_synth_stream_create(&s, h);
    struct G { redio_pfb_synth *h; redio_pfb_synth_stream *s; ~G() { redio_pfb_synth_stream_destroy(s); redio_pfb_synth_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_pfb_synth_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_pfb_synth_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

// the oversampled channelizer (redio_pfb_os_*: a row of nchan channels every hop <= nchan samples, the branch sums turned by
// ((F + r) hop) mod nchan places in front of the transform) as a block.  Per message: every message is a stream of
// its own, its first row is row F = 0.  one_kernel: REDIO_PFB_OS_BLOCK, the workgroup kernel (route 2) where the shape has one.
inline void oversampled_channelizer(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                                    int taps_per_branch, size_t hop, bool fused, bool one_kernel = false)
{
    using cf = std::complex<float>;
    redio_pfb_os *h = nullptr;
    check(redio_pfb_os_create(&h, proto.data(), nchan, taps_per_branch, hop, (fused ? REDIO_FIR_FUSED : 0) | (one_kernel ? REDIO_PFB_OS_BLOCK : 0)));
    struct G { redio_pfb_os *h; ~G() { redio_pfb_os_destroy(h); } } g{h};
    detail::run_block<cf, cf>(u, v, [&](const View<cf> &d) { return redio_pfb_os_nrows(h, d.len) * (size_t)nchan; },
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_pfb_os_enqueue(h, d.data(), d.len, 0, o.data(), st); });
}

// ... and as a stream: messages of any length, the unconsumed samples and the running row index carried, whole rows sent
inline void oversampled_channelizer_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                                           int taps_per_branch, size_t hop, bool fused, bool one_kernel = false)
{
    using cf = std::complex<float>;
    redio_pfb_os *h = nullptr;
    check(redio_pfb_os_create(&h, proto.data(), nchan, taps_per_branch, hop, (fused ? REDIO_FIR_FUSED : 0) | (one_kernel ? REDIO_PFB_OS_BLOCK : 0)));
    redio_pfb_os_stream *s = nullptr;
    const int rc = redio_pfb_os_stream_create(&s, h);
    struct G { redio_pfb_os *h; redio_pfb_os_stream *s; ~G() { redio_pfb_os_stream_destroy(s); redio_pfb_os_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_pfb_os_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_pfb_os_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

// the oversampled synthesis bank (redio_pfb_os_synth_*: the inverse transform of every row of nchan channel values, then a weighted
// overlap-add at hop <= nchan) as a block.  Per message: every message is a stream of its own, its first row is row F = 0.
inline void oversampled_synthesizer(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                                    int taps_per_branch, size_t hop, bool fused)
{
    using cf = std::complex<float>;
    redio_pfb_os_synth *h = nullptr;
    check(redio_pfb_os_synth_create(&h, proto.data(), nchan, taps_per_branch, hop, fused ? REDIO_FIR_FUSED : 0));
    struct G { redio_pfb_os_synth *h; ~G() { redio_pfb_os_synth_destroy(h); } } g{h};
    detail::run_block<cf, cf>(u, v, [&](const View<cf> &d) { return redio_pfb_os_synth_nout(h, d.len); },
                              [&](const View<cf> &d, const View<cf> &o, void *st) { return redio_pfb_os_synth_enqueue(h, d.data(), d.len, 0, o.data(), st); });
}

// ... and as a stream: messages of any length, the unconsumed rows and the running row index carried, whole hops of samples sent
inline void oversampled_synthesizer_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> proto, int nchan,
                                           int taps_per_branch, size_t hop, bool fused)
{
    using cf = std::complex<float>;
    redio_pfb_os_synth *h = nullptr;
    check(redio_pfb_os_synth_create(&h, proto.data(), nchan, taps_per_branch, hop, fused ? REDIO_FIR_FUSED : 0));
    redio_pfb_os_synth_stream *s = nullptr;
    const int rc = redio_pfb_os_synth_stream_create(&s, h);
    struct G { redio_pfb_os_synth *h; redio_pfb_os_synth_stream *s; ~G() { redio_pfb_os_synth_stream_destroy(s); redio_pfb_os_synth_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_pfb_os_synth_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_pfb_os_synth_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

inline void overlap_save_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<float> taps, int nfft)
{
    using cf = std::complex<float>;
    redio_ovsave *h = nullptr;
    check(redio_ovsave_create(&h, taps.data(), taps.size(), nfft));
    redio_ovsave_stream *s = nullptr;
    const int rc = redio_ovsave_stream_create(&s, h);
    struct G { redio_ovsave *h; redio_ovsave_stream *s; ~G() { redio_ovsave_stream_destroy(s); redio_ovsave_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block(u, v, [&](size_t len) { return redio_ovsave_stream_nout(s, len); },
                             [&](const View<cf> &d, cf *o, size_t *got, void *st) { return redio_ovsave_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

// overlap-save on a REAL stream (redio_ovsave_real_*: kiss_fftr / kiss_fftri blocks of nfft samples; an even tap count counts as one
// more), dsputils::convolve's valid-mode semantics per message
inline void overlap_save_real(Receiver<View<float>> u, Sender<View<float>> v, std::vector<float> taps, int nfft)
{
    redio_ovsave_real *h = nullptr;
    check(redio_ovsave_real_create(&h, taps.data(), taps.size(), nfft));
    struct G { redio_ovsave_real *h; ~G() { redio_ovsave_real_destroy(h); } } g{h};
    detail::run_block<float, float>(u, v, [&](const View<float> &d) { return redio_ovsave_real_nout(h, d.len); },
                                    [&](const View<float> &d, const View<float> &o, void *st) { return redio_ovsave_real_enqueue(h, d.data(), d.len, o.data(), st); });
}

// the same as a STREAM: messages of any length, odd ones included, give the outputs of one call on the whole stream
inline void overlap_save_real_stream(Receiver<View<float>> u, Sender<View<float>> v, std::vector<float> taps, int nfft)
{
    redio_ovsave_real *h = nullptr;
    check(redio_ovsave_real_create(&h, taps.data(), taps.size(), nfft));
    redio_ovsave_real_stream *s = nullptr;
    const int rc = redio_ovsave_real_stream_create(&s, h);
    struct G { redio_ovsave_real *h; redio_ovsave_real_stream *s; ~G() { redio_ovsave_real_stream_destroy(s); redio_ovsave_real_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block_of<float, float>(u, v, [&](size_t len) { return redio_ovsave_real_stream_nout(s, len); },
                                              [&](const View<float> &d, float *o, size_t *got, void *st) { return redio_ovsave_real_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

namespace detail {
// what the six power-spectrum blocks differ in: the plan's functions, a message's element type and how many of them make a sample
struct PspecCf32 {
    using In = std::complex<float>; using Plan = redio_pspec; using Stream = redio_pspec_stream;
    static constexpr size_t per_sample = 1;
    static constexpr auto create = redio_pspec_create;
    static constexpr auto destroy = redio_pspec_destroy;
    static constexpr auto nrows = redio_pspec_nrows;
    static constexpr auto enqueue = redio_pspec_enqueue;
    static constexpr auto stream_create = redio_pspec_stream_create;
    static constexpr auto stream_destroy = redio_pspec_stream_destroy;
    static constexpr auto stream_nout = redio_pspec_stream_nout;
    static constexpr auto stream_enqueue = redio_pspec_stream_enqueue;
    static size_t bins(const Plan *, int nfft) { return (size_t)nfft; }
};
struct PspecU8 : PspecCf32 { // a message holds whole samples (an even byte count); the stream carries its history as bytes
    using In = uint8_t;
    static constexpr size_t per_sample = 2;
    static constexpr auto enqueue = redio_pspec_enqueue_u8;
    static constexpr auto stream_create = redio_pspec_stream_create_u8;
};
struct PspecReal {
    using In = float; using Plan = redio_pspec_real; using Stream = redio_pspec_real_stream;
    static constexpr size_t per_sample = 1;
    static constexpr auto create = redio_pspec_real_create;
    static constexpr auto destroy = redio_pspec_real_destroy;
    static constexpr auto nrows = redio_pspec_real_nrows;
    static constexpr auto enqueue = redio_pspec_real_enqueue;
    static constexpr auto stream_create = redio_pspec_real_stream_create;
    static constexpr auto stream_destroy = redio_pspec_real_stream_destroy;
    static constexpr auto stream_nout = redio_pspec_real_stream_nout;
    static constexpr auto stream_enqueue = redio_pspec_real_stream_enqueue;
    static size_t bins(const Plan *h, int) { return redio_pspec_real_nbins(h); }
};

// per-message semantics: the rows that fit in each message, a trailing partial row dropped
template <typename T>
void pspec_block(Receiver<View<typename T::In>> &u, Sender<View<float>> &v, int nfft, size_t integrate, size_t step, const std::vector<float> &window)
{
    using In = typename T::In;
    typename T::Plan *h = nullptr;
    check(T::create(&h, nfft, integrate, step, window.empty() ? nullptr : window.data()));
    struct G { typename T::Plan *h; ~G() { T::destroy(h); } } g{h};
    run_block<In, float>(u, v, [&](const View<In> &d) { return T::nrows(h, d.len / T::per_sample) * T::bins(h, nfft); },
                         [&](const View<In> &d, const View<float> &o, void *st) { return T::enqueue(h, d.data(), d.len, o.data(), st); });
}

// a STREAM: messages of any length give the rows of one call on the whole stream; a message that completes no row sends nothing
template <typename T>
void pspec_stream_block(Receiver<View<typename T::In>> &u, Sender<View<float>> &v, int nfft, size_t integrate, size_t step, const std::vector<float> &window)
{
    using In = typename T::In;
    typename T::Plan *h = nullptr;
    check(T::create(&h, nfft, integrate, step, window.empty() ? nullptr : window.data()));
    typename T::Stream *s = nullptr;
    const int rc = T::stream_create(&s, h);
    struct G { typename T::Plan *h; typename T::Stream *s; ~G() { T::stream_destroy(s); T::destroy(h); } } g{h, s};
    check(rc);
    run_stream_block_of<In, float>(u, v, [&](size_t len) { return T::stream_nout(s, len / T::per_sample); },
                                   [&](const View<In> &d, float *o, size_t *got, void *st) {
                                       if (d.len % T::per_sample) return (int)REDIO_ERR_ARG;
                                       return T::stream_enqueue(s, d.data(), d.len / T::per_sample, o, got, st);
                                   });
}
} // namespace detail

// the integrated power spectrum (redio_pspec_*: |X|^2 of nfft-point kissfft::fft blocks that start every `step` samples, summed over
// `integrate` transforms; window: empty or nfft values): cf32 messages in, rows of nfft f32 out, per-message semantics -- the rows
// that fit in each message, a trailing partial row dropped
inline void power_spectrum(Receiver<View<std::complex<float>>> u, Sender<View<float>> v, int nfft, size_t integrate, size_t step, std::vector<float> window = {}) { detail::pspec_block<detail::PspecCf32>(u, v, nfft, integrate, step, window); }
// the same as a STREAM: messages of any length give the rows of one call on the whole stream; a message that completes no row sends nothing
inline void power_spectrum_stream(Receiver<View<std::complex<float>>> u, Sender<View<float>> v, int nfft, size_t integrate, size_t step, std::vector<float> window = {}) { detail::pspec_stream_block<detail::PspecCf32>(u, v, nfft, integrate, step, window); }

// the receiver's messages straight into the power spectrum: u8 I/Q bytes (rtlsdr::rtlSource, rtlsdr.rs:127-152) -> data_to_samples
// (rtlsdr.rs:159-162) -> the block above, without the cf32 intermediate (redio_pspec_enqueue_u8: ONE kernel at nfft = 1024); a
// message holds whole samples (an even byte count)
inline void power_spectrum_u8(Receiver<View<uint8_t>> u, Sender<View<float>> v, int nfft, size_t integrate, size_t step, std::vector<float> window = {}) { detail::pspec_block<detail::PspecU8>(u, v, nfft, integrate, step, window); }
// the same as a STREAM (redio_pspec_stream_create_u8: the history is carried as bytes)
inline void power_spectrum_stream_u8(Receiver<View<uint8_t>> u, Sender<View<float>> v, int nfft, size_t integrate, size_t step, std::vector<float> window = {}) { detail::pspec_stream_block<detail::PspecU8>(u, v, nfft, integrate, step, window); }

// the real-input integrated power spectrum (redio_pspec_real_*: |X|^2 of nfft-point kiss_fftr rows that start every `step` real
// samples, summed over `integrate` transforms; window: empty or nfft values): f32 messages in, rows of nfft / 2 + 1 f32 out,
// per-message semantics
inline void power_spectrum_real(Receiver<View<float>> u, Sender<View<float>> v, int nfft, size_t integrate, size_t step, std::vector<float> window = {}) { detail::pspec_block<detail::PspecReal>(u, v, nfft, integrate, step, window); }
// the same as a STREAM: messages of any length, odd ones included, give the rows of one call on the whole stream
inline void power_spectrum_real_stream(Receiver<View<float>> u, Sender<View<float>> v, int nfft, size_t integrate, size_t step, std::vector<float> window = {}) { detail::pspec_stream_block<detail::PspecReal>(u, v, nfft, integrate, step, window); }

namespace detail {
// the polyphase spectrometer's four blocks: cf32 or u8 I/Q messages in (per_sample elements make a sample), rows of nchan f32 out
struct PfbSpecCf32 {
    using In = std::complex<float>;
    static constexpr size_t per_sample = 1;
    static constexpr auto enqueue = redio_pfb_pspec_enqueue;
    static constexpr auto stream_create = redio_pfb_pspec_stream_create;
};
struct PfbSpecU8 {
    using In = uint8_t;
    static constexpr size_t per_sample = 2;
    static constexpr auto enqueue = redio_pfb_pspec_enqueue_u8;
    static constexpr auto stream_create = redio_pfb_pspec_stream_create_u8;
};
template <typename T>
void pfb_pspec_block(Receiver<View<typename T::In>> &u, Sender<View<float>> &v, const std::vector<float> &proto, int nchan, int taps_per_branch, size_t integrate, unsigned flags)
{
    using In = typename T::In;
    if (proto.size() != (size_t)nchan * (size_t)taps_per_branch) check(REDIO_ERR_ARG);
    redio_pfb_pspec *h = nullptr;
    check(redio_pfb_pspec_create(&h, proto.data(), nchan, taps_per_branch, integrate, flags));
    struct G { redio_pfb_pspec *h; ~G() { redio_pfb_pspec_destroy(h); } } g{h};
    run_block<In, float>(u, v, [&](const View<In> &d) { return redio_pfb_pspec_nrows(h, d.len / T::per_sample) * (size_t)nchan; },
                         [&](const View<In> &d, const View<float> &o, void *st) { return T::enqueue(h, d.data(), d.len, o.data(), st); });
}
template <typename T>
void pfb_pspec_stream_block(Receiver<View<typename T::In>> &u, Sender<View<float>> &v, const std::vector<float> &proto, int nchan, int taps_per_branch, size_t integrate,
                            unsigned flags)
{
    using In = typename T::In;
    if (proto.size() != (size_t)nchan * (size_t)taps_per_branch) check(REDIO_ERR_ARG);
    redio_pfb_pspec *h = nullptr;
    check(redio_pfb_pspec_create(&h, proto.data(), nchan, taps_per_branch, integrate, flags));
    redio_pfb_pspec_stream *s = nullptr;
    const int rc = T::stream_create(&s, h);
    struct G { redio_pfb_pspec *h; redio_pfb_pspec_stream *s; ~G() { redio_pfb_pspec_stream_destroy(s); redio_pfb_pspec_destroy(h); } } g{h, s};
    check(rc);
    run_stream_block_of<In, float>(u, v, [&](size_t len) { return redio_pfb_pspec_stream_nout(s, len / T::per_sample); },
                                   [&](const View<In> &d, float *o, size_t *got, void *st) {
                                       if (d.len % T::per_sample) return (int)REDIO_ERR_ARG;
                                       return redio_pfb_pspec_stream_enqueue(s, d.data(), d.len / T::per_sample, o, got, st);
                                   });
}
} // namespace detail

// the polyphase spectrometer (redio_pfb_pspec_*: |row[c]|^2 of the nchan-channel polyphase channelizer's rows, summed over `integrate`
// rows; proto: nchan * taps_per_branch prototype taps; flags: REDIO_FIR_FUSED or 0, or-ed with REDIO_PFB_PSPEC_BLOCK for the plan's
// workgroup kernel at 32 / 128 / 256 / 512 / 1024 channels -- all four blocks hand `flags` to redio_pfb_pspec_create as it is): cf32
// messages in, rows of nchan f32 out, per-message semantics -- the rows that fit in each message, a trailing partial row dropped
inline void polyphase_spectrum(Receiver<View<std::complex<float>>> u, Sender<View<float>> v, std::vector<float> proto, int nchan, int taps_per_branch, size_t integrate, unsigned flags = REDIO_FIR_FUSED) { detail::pfb_pspec_block<detail::PfbSpecCf32>(u, v, proto, nchan, taps_per_branch, integrate, flags); }
// the same as a STREAM: messages of any length give the rows of one call on the whole stream; a message that completes no row sends nothing
inline void polyphase_spectrum_stream(Receiver<View<std::complex<float>>> u, Sender<View<float>> v, std::vector<float> proto, int nchan, int taps_per_branch, size_t integrate, unsigned flags = REDIO_FIR_FUSED) { detail::pfb_pspec_stream_block<detail::PfbSpecCf32>(u, v, proto, nchan, taps_per_branch, integrate, flags); }
// the receiver's messages straight into the spectrometer: u8 I/Q bytes (rtlsdr.rs:127-162), without the cf32 intermediate
// (redio_pfb_pspec_enqueue_u8: ONE kernel at 64 channels x 4 / 8 / 16 taps per branch); a message holds whole samples
inline void polyphase_spectrum_u8(Receiver<View<uint8_t>> u, Sender<View<float>> v, std::vector<float> proto, int nchan, int taps_per_branch, size_t integrate, unsigned flags = REDIO_FIR_FUSED) { detail::pfb_pspec_block<detail::PfbSpecU8>(u, v, proto, nchan, taps_per_branch, integrate, flags); }
// the same as a STREAM (redio_pfb_pspec_stream_create_u8: the history is carried as bytes)
inline void polyphase_spectrum_stream_u8(Receiver<View<uint8_t>> u, Sender<View<float>> v, std::vector<float> proto, int nchan, int taps_per_branch, size_t integrate, unsigned flags = REDIO_FIR_FUSED) { detail::pfb_pspec_stream_block<detail::PfbSpecU8>(u, v, proto, nchan, taps_per_branch, integrate, flags); }

namespace detail {
// the tuner's four blocks: cf32 or u8 I/Q messages in (per_sample elements make a sample), cf32 out
struct TunerCf32 {
    using In = std::complex<float>;
    static constexpr size_t per_sample = 1;
    static constexpr auto enqueue = redio_ddc_enqueue;
    static constexpr auto stream_create = redio_ddc_stream_create;
};
struct TunerU8 {
    using In = uint8_t;
    static constexpr size_t per_sample = 2;
    static constexpr auto enqueue = redio_ddc_enqueue_u8;
    static constexpr auto stream_create = redio_ddc_stream_create_u8;
};
inline redio_ddc *tuner_plan(const std::vector<std::complex<float>> &osc, const std::vector<float> &taps, size_t decim, bool fused)
{
    redio_ddc *h = nullptr;
    check(redio_ddc_create(&h, reinterpret_cast<const float *>(osc.data()), osc.size(), taps.data(), taps.size(), decim, fused ? REDIO_FIR_FUSED : 0));
    return h;
}
template <typename T>
void tuner_block(Receiver<View<typename T::In>> &u, Sender<View<std::complex<float>>> &v, const std::vector<std::complex<float>> &osc, const std::vector<float> &taps,
                 size_t decim, bool fused)
{
    using In = typename T::In;
    using cf = std::complex<float>;
    redio_ddc *h = tuner_plan(osc, taps, decim, fused);
    struct G { redio_ddc *h; ~G() { redio_ddc_destroy(h); } } g{h};
    // every message starts the table at entry 0: mul_vecs multiplies EVERY message by the same constant vector (kpn.rs:198-203)
    run_block<In, cf>(u, v, [&](const View<In> &d) { return redio_ddc_nout(h, d.len / T::per_sample); },
                      [&](const View<In> &d, const View<cf> &o, void *st) { return T::enqueue(h, d.data(), d.len, 0, o.data(), st); });
}
template <typename T>
void tuner_stream_block(Receiver<View<typename T::In>> &u, Sender<View<std::complex<float>>> &v, const std::vector<std::complex<float>> &osc,
                        const std::vector<float> &taps, size_t decim, bool fused)
{
    using In = typename T::In;
    using cf = std::complex<float>;
    redio_ddc *h = tuner_plan(osc, taps, decim, fused);
    redio_ddc_stream *s = nullptr;
    const int rc = T::stream_create(&s, h);
    struct G { redio_ddc *h; redio_ddc_stream *s; ~G() { redio_ddc_stream_destroy(s); redio_ddc_destroy(h); } } g{h, s};
    check(rc);
    run_stream_block_of<In, cf>(u, v, [&](size_t len) { return redio_ddc_stream_nout(s, len / T::per_sample); },
                                [&](const View<In> &d, cf *o, size_t *got, void *st) {
                                    if (d.len % T::per_sample) return (int)REDIO_ERR_ARG;
                                    return redio_ddc_stream_enqueue(s, d.data(), d.len / T::per_sample, o, got, st);
                                });
}
} // namespace detail

// the tuner (redio_ddc_*: kpn::mul_vecs by the periodic table `osc`, kpn.rs:198-203, fused into the FIR of dsputils::convolve,
// dsputils.rs:30-32, with decimation): cf32 messages in, cf32 out, per-message semantics -- the table restarts at entry 0 with every
// message, exactly as mul_vecs multiplies every message by the same vector, and ntaps - 1 outputs are lost at every seam.  Queue-ordered
// on the rings like dev::fir.
inline void tuner(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t decim, bool fused) { detail::tuner_block<detail::TunerCf32>(u, v, osc, taps, decim, fused); }
// the receiver's messages straight into the tuner: u8 I/Q bytes (rtlsdr.rs:127-162), without the cf32 intermediate; a message holds whole samples
inline void tuner_u8(Receiver<View<uint8_t>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t decim, bool fused) { detail::tuner_block<detail::TunerU8>(u, v, osc, taps, decim, fused); }
// the same as a STREAM (redio_ddc_stream_*): history AND oscillator phase are carried, so messages of any length give the outputs of one
// call on the whole stream; a message that completes no output sends nothing.  Queue-ordered like dev::fir_stream.
inline void tuner_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t decim, bool fused) { detail::tuner_stream_block<detail::TunerCf32>(u, v, osc, taps, decim, fused); }
inline void tuner_stream_u8(Receiver<View<uint8_t>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t decim, bool fused) { detail::tuner_stream_block<detail::TunerU8>(u, v, osc, taps, decim, fused); }

namespace detail {
// the rational resampler's two blocks: T is float or std::complex<float>, in and out
template <typename T>
redio_upfirdn *upfirdn_plan(const std::vector<float> &taps, size_t up, size_t down, bool fused)
{
    redio_upfirdn *h = nullptr;
    check(redio_upfirdn_create(&h, taps.data(), taps.size(), up, down, (sizeof(T) == 8 ? REDIO_FIR_COMPLEX : 0) | (fused ? REDIO_FIR_FUSED : 0)));
    return h;
}
} // namespace detail

// the rational resampler (redio_upfirdn_*: up by `up`, the FIR of dsputils::convolve, dsputils.rs:30-32, down by `down`, as a polyphase
// FIR over the original samples): f32 or cf32 messages in, the same type out, per-message semantics -- every message starts at phase 0
// and the outputs whose taps would reach past its end are lost at every seam.  Queue-ordered on the rings like dev::fir.
template <typename T>
void upfirdn(Receiver<View<T>> u, Sender<View<T>> v, std::vector<float> taps, size_t up, size_t down, bool fused)
{
    redio_upfirdn *h = detail::upfirdn_plan<T>(taps, up, down, fused);
    struct G { redio_upfirdn *h; ~G() { redio_upfirdn_destroy(h); } } g{h};
    detail::run_block<T, T>(u, v, [&](const View<T> &d) { return redio_upfirdn_nout(h, d.len); },
                            [&](const View<T> &d, const View<T> &o, void *st) { return redio_upfirdn_enqueue(h, d.data(), d.len, o.data(), st); });
}
// the same as a STREAM (redio_upfirdn_stream_*): the history is carried, so messages of any length give whole periods of the outputs of
// one call on the whole stream; a message that completes no period sends nothing.  Queue-ordered like dev::fir_stream.
template <typename T>
void upfirdn_stream(Receiver<View<T>> u, Sender<View<T>> v, std::vector<float> taps, size_t up, size_t down, bool fused)
{
    redio_upfirdn *h = detail::upfirdn_plan<T>(taps, up, down, fused);
    redio_upfirdn_stream *s = nullptr;
    const int rc = redio_upfirdn_stream_create(&s, h);
    struct G { redio_upfirdn *h; redio_upfirdn_stream *s; ~G() { redio_upfirdn_stream_destroy(s); redio_upfirdn_destroy(h); } } g{h, s};
    check(rc);
    detail::run_stream_block_of<T, T>(u, v, [&](size_t len) { return redio_upfirdn_stream_nout(s, len); },
                                      [&](const View<T> &d, T *o, size_t *got, void *st) { return redio_upfirdn_stream_enqueue(s, d.data(), d.len, o, got, st); });
}

namespace detail {
// the tuned resampler's four blocks: cf32 or u8 I/Q messages in (per_sample elements make a sample), cf32 out
struct TunedResamplerCf32 {
    using In = std::complex<float>;
    static constexpr size_t per_sample = 1;
    static constexpr auto enqueue = redio_ddc_upfirdn_enqueue;
    static constexpr auto stream_create = redio_ddc_upfirdn_stream_create;
};
struct TunedResamplerU8 {
    using In = uint8_t;
    static constexpr size_t per_sample = 2;
    static constexpr auto enqueue = redio_ddc_upfirdn_enqueue_u8;
    static constexpr auto stream_create = redio_ddc_upfirdn_stream_create_u8;
};
inline redio_ddc_upfirdn *tuned_resampler_plan(const std::vector<std::complex<float>> &osc, const std::vector<float> &taps, size_t up, size_t down, bool fused)
{
    redio_ddc_upfirdn *h = nullptr;
    check(redio_ddc_upfirdn_create(&h, reinterpret_cast<const float *>(osc.data()), osc.size(), taps.data(), taps.size(), up, down, fused ? REDIO_FIR_FUSED : 0));
    return h;
}
template <typename T>
void tuned_resampler_block(Receiver<View<typename T::In>> &u, Sender<View<std::complex<float>>> &v, const std::vector<std::complex<float>> &osc,
                           const std::vector<float> &taps, size_t up, size_t down, bool fused)
{
    using In = typename T::In;
    using cf = std::complex<float>;
    redio_ddc_upfirdn *h = tuned_resampler_plan(osc, taps, up, down, fused);
    struct G { redio_ddc_upfirdn *h; ~G() { redio_ddc_upfirdn_destroy(h); } } g{h};
    // every message starts the table at entry 0 and the resampler at phase 0, as dev::tuner and dev::upfirdn do
    run_block<In, cf>(u, v, [&](const View<In> &d) { return redio_ddc_upfirdn_nout(h, d.len / T::per_sample); },
                      [&](const View<In> &d, const View<cf> &o, void *st) { return T::enqueue(h, d.data(), d.len, 0, o.data(), st); });
}
template <typename T>
void tuned_resampler_stream_block(Receiver<View<typename T::In>> &u, Sender<View<std::complex<float>>> &v, const std::vector<std::complex<float>> &osc,
                                  const std::vector<float> &taps, size_t up, size_t down, bool fused)
{
    using In = typename T::In;
    using cf = std::complex<float>;
    redio_ddc_upfirdn *h = tuned_resampler_plan(osc, taps, up, down, fused);
    redio_ddc_upfirdn_stream *s = nullptr;
    const int rc = T::stream_create(&s, h);
    struct G { redio_ddc_upfirdn *h; redio_ddc_upfirdn_stream *s; ~G() { redio_ddc_upfirdn_stream_destroy(s); redio_ddc_upfirdn_destroy(h); } } g{h, s};
    check(rc);
    run_stream_block_of<In, cf>(u, v, [&](size_t len) { return redio_ddc_upfirdn_stream_nout(s, len / T::per_sample); },
                                [&](const View<In> &d, cf *o, size_t *got, void *st) {
                                    if (d.len % T::per_sample) return (int)REDIO_ERR_ARG;
                                    return redio_ddc_upfirdn_stream_enqueue(s, d.data(), d.len / T::per_sample, o, got, st);
                                });
}
} // namespace detail

// the tuned resampler (redio_ddc_upfirdn_*: kpn::mul_vecs by the periodic table `osc`, kpn.rs:198-203, fused into the tile load of the
// rational resampler, the polyphase form of dsputils::convolve, dsputils.rs:30-32): cf32 messages in, cf32 out, per-message semantics --
// the table restarts at entry 0 and the resampler at phase 0 with every message, and the outputs whose taps would reach past its end are
// lost at every seam.  Queue-ordered on the rings like dev::fir.
inline void tuned_resampler(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t up, size_t down, bool fused) { detail::tuned_resampler_block<detail::TunedResamplerCf32>(u, v, osc, taps, up, down, fused); }
// the receiver's messages straight into it: u8 I/Q bytes (rtlsdr.rs:127-162), without the cf32 intermediate; a message holds whole samples
inline void tuned_resampler_u8(Receiver<View<uint8_t>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t up, size_t down, bool fused) { detail::tuned_resampler_block<detail::TunedResamplerU8>(u, v, osc, taps, up, down, fused); }
// the same as a STREAM (redio_ddc_upfirdn_stream_*): history AND oscillator phase are carried, so messages of any length give whole
// periods of the outputs of one call on the whole stream; a message that completes no period sends nothing.  Queue-ordered like dev::fir_stream.
inline void tuned_resampler_stream(Receiver<View<std::complex<float>>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t up, size_t down, bool fused) { detail::tuned_resampler_stream_block<detail::TunedResamplerCf32>(u, v, osc, taps, up, down, fused); }
inline void tuned_resampler_stream_u8(Receiver<View<uint8_t>> u, Sender<View<std::complex<float>>> v, std::vector<std::complex<float>> osc, std::vector<float> taps, size_t up, size_t down, bool fused) { detail::tuned_resampler_stream_block<detail::TunedResamplerU8>(u, v, osc, taps, up, down, fused); }

} // namespace dev
} // namespace kpn
