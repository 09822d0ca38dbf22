// kpn_list_tests.cpp -- the list launches (redio_chain_enqueue_list, redio_fft_enqueue_list) and the coalescing blocks of
// include/kpn_dev.hpp (dev::set_coalesce_limit).
//   kpn_list_tests list_plumbing          CPU only: detail::run_block_list on host memory through the dev::DeviceApi stand-ins
//   kpn_list_tests list_gpu               source -> dev::fir_fft_chain and 1024-sample source -> dev::fft into the checksum sink, coalescing
//                                         off and on: one line "list_gpu <graph> off <sum> <msgs> on <sum> <msgs>" per graph
//   kpn_list_tests bench_list log2_msg k  one JSON line: bare single launches against bare list launches of k messages (interleaved),
//                                         and the graph (resident source -> dev::fir_fft_chain -> drop / checksum sink) coalescing off
//                                         against on
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace kpn;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (line %d)\n", #c, __LINE__); return 1; } } while (0)

// ---- host-memory stand-ins for dev::DeviceApi (as tests/cpp/kpn_tests.cpp's): the coalescing loop runs without a GPU ----
namespace fake {
static std::atomic<long> mallocs{0}, frees{0};
struct St { int dummy; };
static int malloc_(void **p, size_t b) { *p = std::malloc(b ? b : 1); ++mallocs; return *p ? 0 : REDIO_ERR_NOMEM; }
static int free_(void *p) { std::free(p); ++frees; return 0; }
static int ev_create(void **e) { *e = new int(0); return 0; }
static int ev_destroy(void *e) { delete (int *)e; return 0; }
static int ev_record(void *, void *) { return 0; }
static int ev_wait(void *, void *) { return 0; }
static int st_create(void **s) { *s = new St; return 0; }
static int st_destroy(void *s) { delete (St *)s; return 0; }
static int st_sync(void *) { return 0; }
static int get_device(int *d) { *d = 0; return 0; }
struct Install {
    dev::DeviceApi saved;
    Install() : saved(dev::api())
    {
        auto &a = dev::api();
        a.malloc_ = malloc_; a.free_ = free_; a.event_create = ev_create; a.event_destroy = ev_destroy; a.event_record = ev_record;
        a.stream_wait_event = ev_wait; a.stream_create = st_create; a.stream_destroy = st_destroy; a.stream_sync = st_sync; a.get_device = get_device;
    }
    ~Install() { dev::api() = saved; }
};
} // namespace fake

// the block under test: message i (ints) -> nout = len + (len % 3) ints, out[j] = in[j % len] * 3 + j, via ONE host "list launch" per batch
struct HostBlock {
    std::atomic<size_t> batches{0}, messages{0}, largest{0};
    void run(Receiver<dev::View<int>> u, Sender<dev::View<int>> v, size_t limit)
    {
        dev::detail::run_block_list<int, int>(u, v, [](const dev::View<int> &d) { return d.len + d.len % 3; },
                                              [&](const std::vector<dev::View<int>> &ds, const dev::View<int> &o, const std::vector<size_t> &offs, void *) {
                                                  for (size_t i = 0; i < ds.size(); ++i) {
                                                      if (offs[i] % 64) return REDIO_ERR_ARG; // 256-byte offsets
                                                      const size_t n = ds[i].len + ds[i].len % 3;
                                                      for (size_t j = 0; j < n; ++j) o.data()[offs[i] + j] = ds[i].data()[j % ds[i].len] * 3 + (int)j;
                                                  }
                                                  ++batches;
                                                  messages += ds.size();
                                                  size_t l = largest.load();
                                                  while (ds.size() > l && !largest.compare_exchange_weak(l, ds.size())) {}
                                                  return REDIO_OK;
                                              }, limit);
    }
};
static size_t plen(size_t i) { return 1 + (i * 37) % 300; }
static int pval(size_t i, size_t j) { return (int)(i * 1000 + j); }
static dev::View<int> pmsg(size_t i)
{
    auto d = dev::make<int>(plen(i));
    for (size_t j = 0; j < d.len; ++j) d.data()[j] = pval(i, j);
    return d;
}
static bool pcheck(size_t i, const dev::View<int> &o)
{
    const size_t len = plen(i);
    if (o.len != len + len % 3) return false;
    for (size_t j = 0; j < o.len; ++j) if (o.data()[j] != pval(i, j % len) * 3 + (int)j) return false;
    return true;
}

static int list_plumbing()
{
    fake::Install inst;
    { // all messages queued before the block starts: batches of `limit` form; order, boundaries and contents hold; the ring bounds memory
        const size_t N = 200, limit = 8;
        auto [s1, r1] = channel<dev::View<int>>();
        auto [s2, r2] = channel<dev::View<int>>();
        for (size_t i = 0; i < N; ++i) s1.send_unwrap(pmsg(i));
        { auto drop = std::move(s1); }
        const long m0 = fake::mallocs.load();
        HostBlock b;
        std::thread t([&, r = std::move(r1), s = std::move(s2)]() mutable { try { b.run(std::move(r), std::move(s), limit); } catch (const hangup &) {} });
        size_t got = 0;
        while (auto o = r2.try_recv_blocking()) { CHECK(pcheck(got, *o)); ++got; }
        t.join();
        CHECK(got == N && b.messages.load() == N);
        CHECK(b.largest.load() == limit && b.batches.load() == (N + limit - 1) / limit);
        CHECK(fake::mallocs.load() - m0 <= (long)(2 * dev::default_ring_depth_ref().load())); // ring buffers only, not one per message
    }
    { // limit 1: today's loop, one launch per message
        auto [s1, r1] = channel<dev::View<int>>();
        auto [s2, r2] = channel<dev::View<int>>();
        for (size_t i = 0; i < 20; ++i) s1.send_unwrap(pmsg(i));
        { auto drop = std::move(s1); }
        HostBlock b;
        std::thread t([&, r = std::move(r1), s = std::move(s2)]() mutable { try { b.run(std::move(r), std::move(s), 1); } catch (const hangup &) {} });
        size_t got = 0;
        while (auto o = r2.try_recv_blocking()) { CHECK(pcheck(got, *o)); ++got; }
        t.join();
        CHECK(got == 20 && b.batches.load() == 20 && b.largest.load() == 1);
    }
    { // a consumer that holds every output: the block stalls at the ring's depth (credits), resumes as handles drop
        const size_t depth = 2, limit = 4;
        dev::set_default_ring_depth(depth);
        auto [s1, r1] = channel<dev::View<int>>();
        auto [s2, r2] = channel<dev::View<int>>();
        for (size_t i = 0; i < 40; ++i) s1.send_unwrap(pmsg(i));
        { auto drop = std::move(s1); }
        HostBlock b;
        std::thread t([&, r = std::move(r1), s = std::move(s2)]() mutable { try { b.run(std::move(r), std::move(s), limit); } catch (const hangup &) {} });
        std::vector<dev::View<int>> held;
        for (size_t i = 0; i < depth * limit; ++i) held.push_back(r2.recv());
        std::this_thread::sleep_for(std::chrono::milliseconds(50));
        CHECK(b.batches.load() == depth); // both buffers out: no third batch
        for (size_t i = 0; i < held.size(); ++i) CHECK(pcheck(i, held[i]));
        held.clear();
        size_t got = depth * limit;
        while (auto o = r2.try_recv_blocking()) { CHECK(pcheck(got, *o)); ++got; }
        t.join();
        CHECK(got == 40);
        dev::set_default_ring_depth(4);
    }
    { // hang-up with a batch open: the 5 collected messages still go out, then the block ends
        auto [s1, r1] = channel<dev::View<int>>();
        auto [s2, r2] = channel<dev::View<int>>();
        for (size_t i = 0; i < 5; ++i) s1.send_unwrap(pmsg(i));
        { auto drop = std::move(s1); }
        HostBlock b;
        bool ended = false;
        std::thread t([&, r = std::move(r1), s = std::move(s2)]() mutable { try { b.run(std::move(r), std::move(s), 8); } catch (const hangup &) { ended = true; } });
        size_t got = 0;
        while (auto o = r2.try_recv_blocking()) { CHECK(pcheck(got, *o)); ++got; }
        t.join();
        CHECK(ended && got == 5 && b.batches.load() == 1);
    }
    { // a producer whose ring holds ONE buffer: it waits for each message's handle, so the block never finds a second message queued --
      // it must not wait for one (no deadlock), and runs batches of one
        const size_t N = 50;
        auto [s1, r1] = bounded_channel<dev::View<int>>(4);
        auto [s2, r2] = channel<dev::View<int>>();
        std::thread prod([s = std::move(s1)]() mutable {
            dev::BlockStream st;
            dev::Ring ring(1);
            for (size_t i = 0; i < N; ++i) {
                auto d = ring.acquire<int>(plen(i), st);
                for (size_t j = 0; j < d.len; ++j) d.data()[j] = pval(i, j);
                dev::publish(d, st);
                s.send_unwrap(std::move(d));
            }
        });
        HostBlock b;
        std::atomic<bool> done{false};
        std::thread t([&, r = std::move(r1), s = std::move(s2)]() mutable { try { b.run(std::move(r), std::move(s), 8); } catch (const hangup &) {} done = true; });
        size_t got = 0;
        const auto t0 = std::chrono::steady_clock::now();
        while (got < N && std::chrono::steady_clock::now() - t0 < std::chrono::seconds(20)) {
            auto o = r2.try_recv();
            if (!o) { std::this_thread::sleep_for(std::chrono::microseconds(100)); continue; }
            CHECK(pcheck(got, *o));
            ++got;
        }
        CHECK(got == N); // else: deadlock
        prod.join();
        t.join();
        CHECK(done.load() && b.largest.load() == 1);
    }
    CHECK(fake::mallocs.load() == fake::frees.load());
    std::printf("list_plumbing ok\n");
    return 0;
}

// ---- graphs on the GPU ----
using cf = std::complex<float>;
struct GraphRun { unsigned long long sum = 0; size_t msgs = 0; };

// resident ragged messages (views of one buffer, 16-byte aligned) -> block -> checksum sink
template <typename Block>
static GraphRun run_graph(const dev::View<cf> &big, const std::vector<size_t> &offs, const std::vector<size_t> &lens, size_t limit, Block block)
{
    dev::set_coalesce_limit(limit);
    auto [s1, r1] = bounded_channel<dev::View<cf>>(std::max<size_t>(8, 2 * limit));
    auto [s2, r2] = channel<dev::View<cf>>();
    GraphRun g;
    std::thread src([&, s = std::move(s1)]() mutable { for (size_t i = 0; i < lens.size(); ++i) s.send_unwrap(big.sub(offs[i], lens[i])); });
    std::thread blk([&, r = std::move(r1), s = std::move(s2)]() mutable { try { block(std::move(r), std::move(s)); } catch (const hangup &) {} });
    std::thread snk([&, r = std::move(r2)]() mutable { dev::checksum_sink<cf>(std::move(r), &g.sum, &g.msgs); });
    src.join(); blk.join(); snk.join();
    dev::set_coalesce_limit(1);
    return g;
}

static int list_gpu()
{
    const std::vector<float> taps = dsputils::lpf_corrected(127, 0.08f);
    { // chain: ragged messages (no block, one block, several, trailing samples)
        std::vector<size_t> offs, lens;
        size_t pos = 0;
        for (size_t i = 0; i < 150; ++i) {
            const size_t len = (i % 7 == 3) ? 4000 : 5246 + (i % 5) * 5120 + (i % 3) * 77;
            offs.push_back(pos); lens.push_back(len);
            pos += (len + 1) & ~(size_t)1; // even offsets: 16-byte aligned messages
        }
        auto big = dev::make<cf>(pos);
        dev::check(redio_synth_iq(big.data(), 0x5EED0002u, 0, pos, nullptr));
        dev::check(redio_stream_sync(nullptr));
        auto chain = [&](Receiver<dev::View<cf>> r, Sender<dev::View<cf>> s) { dev::fir_fft_chain(std::move(r), std::move(s), taps, 5, 1024, true); };
        const GraphRun off = run_graph(big, offs, lens, 1, chain), on = run_graph(big, offs, lens, 32, chain);
        std::printf("list_gpu chain off %llu %zu on %llu %zu\n", off.sum, off.msgs, on.sum, on.msgs);
    }
    { // FFT: 1024-sample messages
        const size_t N = 300;
        std::vector<size_t> offs, lens;
        for (size_t i = 0; i < N; ++i) { offs.push_back(i * 1024); lens.push_back(1024); }
        auto big = dev::make<cf>(N * 1024);
        dev::check(redio_synth_iq(big.data(), 0x5EED0003u, 0, N * 1024, nullptr));
        dev::check(redio_stream_sync(nullptr));
        auto fft = [&](Receiver<dev::View<cf>> r, Sender<dev::View<cf>> s) { dev::fft(std::move(r), std::move(s), 1024, 0); };
        const GraphRun off = run_graph(big, offs, lens, 1, fft), on = run_graph(big, offs, lens, 32, fft);
        std::printf("list_gpu fft off %llu %zu on %llu %zu\n", off.sum, off.msgs, on.sum, on.msgs);
    }
    return 0;
}

// ---- bench_list ----
using clk = std::chrono::steady_clock;
static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

struct GraphBench { double us_per_msg; double msgs_per_launch; unsigned long long mallocs; unsigned long long sum; };
// resident source (R inputs cycled, a channel of depth >= k to run ahead) -> dev::fir_fft_chain -> sink; the host clock between two
// completed synchronisations after `warm` messages
static GraphBench graph_bench(const dev::View<cf> &big, size_t msg, size_t R, size_t warm, size_t nmsg, size_t limit, bool checksum,
                              const std::vector<float> &taps)
{
    dev::set_coalesce_limit(limit);
    auto [s1, r1] = bounded_channel<dev::View<cf>>(std::max<size_t>(8, 2 * limit));
    auto [s2, r2] = channel<dev::View<cf>>();
    const size_t total = warm + nmsg;
    GraphBench res{};
    clk::time_point t0, t1;
    unsigned long long m0 = 0, m1 = 0;
    size_t batches = 0;
    std::thread src([&, s = std::move(s1)]() mutable { for (size_t i = 0; i < total; ++i) s.send_unwrap(big.sub((i % R) * msg, msg)); });
    std::thread blk([&, r = std::move(r1), s = std::move(s2)]() mutable {
        try { dev::fir_fft_chain(std::move(r), std::move(s), taps, 5, 1024, true); } catch (const hangup &) {}
    });
    std::thread snk([&, r = std::move(r2)]() mutable {
        dev::BlockStream st;
        auto acc = dev::make<unsigned long long>(1);
        const unsigned long long zero = 0;
        dev::check(redio_upload(acc.data(), &zero, 8, st));
        dev::check(redio_stream_sync(st));
        for (size_t i = 0; i < total; ++i) {
            auto d = r.recv();
            if (i >= warm && d.off == 0) ++batches; // the first output of a batch sits at the start of its buffer, the others behind it
            {
                dev::Reading<cf> in(d, st);
                if (checksum && i >= warm) dev::check(redio_checksum_u32(d.data(), d.len * 2, acc.data(), st));
            }
            d = dev::View<cf>();
            if (i + 1 == warm) { dev::check(redio_stream_sync(st)); m0 = redio_malloc_count(); t0 = clk::now(); }
        }
        dev::check(redio_stream_sync(st));
        t1 = clk::now();
        m1 = redio_malloc_count();
        dev::check(redio_download(&res.sum, acc.data(), 8, st));
        dev::check(redio_stream_sync(st));
    });
    src.join(); blk.join(); snk.join();
    dev::set_coalesce_limit(1);
    res.us_per_msg = secs(t0, t1) / (double)nmsg * 1e6;
    res.msgs_per_launch = batches ? (double)nmsg / (double)batches : 0;
    res.mallocs = m1 - m0;
    return res;
}

static int bench_list(int log2_msg, size_t k)
{
    if (k < 1 || k > REDIO_LIST_MAX || log2_msg < 13 || log2_msg > 26) { std::fprintf(stderr, "bench_list: 13 <= log2_msg <= 26, 1 <= k <= 32\n"); return 2; }
    const size_t msg = (size_t)1 << log2_msg, R = 4;
    const std::vector<float> taps = dsputils::lpf_corrected(127, 0.08f);
    auto big = dev::make<cf>(R * msg);
    dev::check(redio_synth_iq(big.data(), 0x5EED0002u, 0, R * msg, nullptr));
    dev::check(redio_stream_sync(nullptr));
    redio_chain *h = nullptr;
    dev::check(redio_chain_create(&h, taps.data(), taps.size(), 5, 1024, REDIO_FIR_FUSED));
    const size_t nblk = redio_chain_nblocks(h, msg), nout = nblk * 1024;
    auto outs = dev::make<cf>(k * nout); // k distinct outputs: a list's outputs must not overlap
    dev::BlockStream st(dev::BlockStream::TRANSFER);
    // bare: n messages as single launches, or as list launches of k; message i reads input i % R and writes output i % k
    auto single = [&](size_t n) {
        for (size_t i = 0; i < n; ++i) dev::check(redio_chain_enqueue(h, big.data() + (i % R) * msg, msg, outs.data() + (i % k) * nout, st));
        dev::check(redio_stream_sync(st));
    };
    auto listed = [&](size_t n) {
        redio_msg m[REDIO_LIST_MAX];
        for (size_t i = 0; i < n; i += k) {
            const size_t c = std::min(k, n - i);
            for (size_t j = 0; j < c; ++j) m[j] = redio_msg{big.data() + ((i + j) % R) * msg, msg, outs.data() + j * nout};
            dev::check(redio_chain_enqueue_list(h, m, c, st));
        }
        dev::check(redio_stream_sync(st));
    };
    single(4 * k);
    listed(4 * k);
    auto t0 = clk::now();
    size_t done = 0;
    while (secs(t0, clk::now()) < 0.1) { single(k); done += k; }
    const double per = secs(t0, clk::now()) / (double)done;
    const size_t nmsg = std::max<size_t>(4 * k, (size_t)(0.25 / per) / k * k); // about 0.25 s per timed run of single launches
    double bare_single = 1e30, bare_list = 1e30;
    for (int rep = 0; rep < 3; ++rep) { // interleaved, best of three
        auto a = clk::now(); single(nmsg); auto b = clk::now(); listed(nmsg); auto c = clk::now();
        bare_single = std::min(bare_single, secs(a, b) / (double)nmsg * 1e6);
        bare_list = std::min(bare_list, secs(b, c) / (double)nmsg * 1e6);
    }
    redio_chain_destroy(h);
    const size_t warm = std::max<size_t>(8, (size_t)(0.1 / per) / k * k), gn = std::max<size_t>(4 * k, (size_t)(0.2 / per) / k * k);
    const GraphBench off_drop = graph_bench(big, msg, R, warm, gn, 1, false, taps), on_drop = graph_bench(big, msg, R, warm, gn, k, false, taps);
    const GraphBench off_sum = graph_bench(big, msg, R, warm, gn, 1, true, taps), on_sum = graph_bench(big, msg, R, warm, gn, k, true, taps);
    const double used = (double)(nblk * 5120);
    std::printf("{\"mode\": \"bench_list\", \"log2_msg\": %d, \"k\": %zu, \"used_samples_per_msg\": %.0f, \"bare_messages\": %zu, \"graph_messages\": %zu, "
                "\"bare_single_us_per_msg\": %.3f, \"bare_list_us_per_msg\": %.3f, \"bare_list_over_single\": %.4f, "
                "\"graph_drop_off_us_per_msg\": %.3f, \"graph_drop_on_us_per_msg\": %.3f, \"graph_drop_on_over_off_rate\": %.4f, "
                "\"graph_checksum_off_us_per_msg\": %.3f, \"graph_checksum_on_us_per_msg\": %.3f, \"graph_checksum_on_over_off_rate\": %.4f, "
                "\"graph_drop_on_gsps\": %.3f, \"graph_drop_off_gsps\": %.3f, \"msgs_per_launch\": %.2f, \"mallocs_in_timed_region\": %llu, "
                "\"checksum_off\": %llu, \"checksum_on\": %llu}\n",
                log2_msg, k, used, nmsg, gn, bare_single, bare_list, bare_list / bare_single,
                off_drop.us_per_msg, on_drop.us_per_msg, off_drop.us_per_msg / on_drop.us_per_msg,
                off_sum.us_per_msg, on_sum.us_per_msg, off_sum.us_per_msg / on_sum.us_per_msg,
                used / on_drop.us_per_msg * 1e-3, used / off_drop.us_per_msg * 1e-3, on_drop.msgs_per_launch,
                off_drop.mallocs + on_drop.mallocs + off_sum.mallocs + on_sum.mallocs, off_sum.sum, on_sum.sum);
    std::fflush(stdout);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "list_plumbing";
        if (mode == "list_plumbing") return list_plumbing();
        if (mode == "list_gpu") return list_gpu();
        if (mode == "bench_list" && argc == 4) return bench_list(std::atoi(argv[2]), (size_t)std::atol(argv[3]));
        std::fprintf(stderr, "usage: kpn_list_tests list_plumbing | list_gpu | bench_list log2_msg k\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
