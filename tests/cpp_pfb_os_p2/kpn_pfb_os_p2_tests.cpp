// kpn_pfb_os_p2_tests.cpp -- the oversampled channelizer's blocks of include/kpn_dev.hpp with one_kernel = true (REDIO_PFB_OS_BLOCK:
// the workgroup kernel, route 2) in a device-resident graph, against the bare redio_pfb_os_* calls on a flagged plan.
//   kpn_pfb_os_p2_tests stream|blocks <depth> <nchan> <taps_per_branch> <hop> <fused> <proto.f32> <input.cf32> <out.bin>
//       source (the file's samples, uploaded message by message) -> dev::oversampled_channelizer_stream / dev::oversampled_channelizer -> sink.
//       Eight messages of (P + 40) M + 101 and (P + 40) M - 37 samples in turn; the first is P + 1 rows of M longer, so that no later
//       message of the stream yields more than it (a ring sizes its buffers on its first message).
// Rings of <depth> buffers; the sink's samples go to <out.bin> in arrival order.  The bare calls: `blocks` is one redio_pfb_os_enqueue
// with first_row = 0 per message, `stream` is ONE call with first_row = 0 on the whole input.
// stdout: "<mode> <depth> route <the bare plan's> msgs <n> samples <n> bare_equal <0|1> mallocs_after_first <n>".
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace kpn;
using cf = std::complex<float>;

static void source(Sender<dev::View<cf>> v, const std::vector<cf> &data, const std::vector<size_t> &lens)
{
    dev::BlockStream st;
    dev::Ring ring;
    size_t first = 0;
    for (size_t len : lens) {
        auto d = ring.acquire<cf>(len, st);
        dev::check(redio_upload(d.data(), data.data() + first, len * sizeof(cf), st));
        dev::publish(d, st);
        v.send_unwrap(std::move(d));
        first += len;
    }
}

static void sink(Receiver<dev::View<cf>> u, std::vector<cf> *all, size_t *msgs, unsigned long long *after_first)
{
    dev::BlockStream st;
    std::vector<cf> host;
    unsigned long long m1 = 0;
    try {
        for (;;) {
            auto d = u.recv();
            host.resize(d.len);
            {
                dev::Reading<cf> in(d, st);
                dev::check(redio_download(host.data(), d.data(), d.len * sizeof(cf), st));
            }
            dev::check(redio_stream_sync(st));
            all->insert(all->end(), host.begin(), host.end());
            if (++*msgs == 1) m1 = redio_malloc_count();
        }
    } catch (const hangup &) {
    }
    *after_first = redio_malloc_count() - m1;
}

template <typename T>
static std::vector<T> read_all(const std::string &path)
{
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    std::vector<T> t;
    T buf[4096];
    size_t n;
    while ((n = std::fread(buf, sizeof(T), 4096, f)) > 0) t.insert(t.end(), buf, buf + n);
    std::fclose(f);
    return t;
}

// what the bare calls give
static std::vector<cf> bare(const std::string &mode, const std::vector<float> &proto, int M, int P, size_t H, bool fused, const std::vector<cf> &data,
                            const std::vector<size_t> &lens, size_t total, int *route)
{
    redio_pfb_os *h = nullptr;
    dev::check(redio_pfb_os_create(&h, proto.data(), M, P, H, (fused ? REDIO_FIR_FUSED : 0) | REDIO_PFB_OS_BLOCK));
    *route = redio_pfb_os_route(h);
    void *d_in = nullptr, *d_out = nullptr, *st = nullptr;
    dev::check(redio_stream_create(&st));
    dev::check(redio_malloc(&d_in, total * sizeof(cf)));
    dev::check(redio_malloc(&d_out, (redio_pfb_os_nrows(h, total) * (size_t)M + 1) * sizeof(cf)));
    dev::check(redio_upload(d_in, data.data(), total * sizeof(cf), st));
    std::vector<cf> out;
    auto one = [&](const void *src, size_t len) {
        const size_t n = redio_pfb_os_nrows(h, len) * (size_t)M;
        dev::check(redio_pfb_os_enqueue(h, src, len, 0, d_out, st));
        const size_t at = out.size();
        out.resize(at + n);
        dev::check(redio_download(out.data() + at, d_out, n * sizeof(cf), st));
        dev::check(redio_stream_sync(st));
    };
    if (mode == "stream") {
        one(d_in, total);
    } else {
        size_t first = 0;
        for (size_t len : lens) { one((const char *)d_in + first * sizeof(cf), len); first += len; }
    }
    redio_free(d_in); redio_free(d_out); redio_stream_destroy(st);
    redio_pfb_os_destroy(h);
    return out;
}

static int run(const std::string &mode, size_t depth, int M, int P, size_t H, bool fused, const std::string &proto_path, const std::string &in_path,
               const char *path)
{
    const std::vector<float> proto = read_all<float>(proto_path);
    const std::vector<cf> data = read_all<cf>(in_path);
    if (proto.size() != (size_t)M * P) { std::fprintf(stderr, "the prototype needs %d taps\n", M * P); return 1; }
    std::vector<size_t> lens;
    size_t total = 0;
    for (int i = 0; i < 8; ++i) lens.push_back((size_t)(P + 40 + (i ? 0 : P + 1)) * M + (i % 2 ? 0 : 101) - (i % 2 ? 37 : 0));
    for (size_t len : lens) total += len;
    if (data.size() < total) { std::fprintf(stderr, "the input file needs %zu samples\n", total); return 1; }
    dev::set_default_ring_depth(depth);
    size_t msgs = 0;
    unsigned long long after_first = 0;
    std::vector<cf> got;
    {
        auto [s1, r1] = bounded_channel<dev::View<cf>>(8);
        auto [s2, r2] = channel<dev::View<cf>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source(std::move(s), data, lens); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
            if (mode == "stream") dev::oversampled_channelizer_stream(std::move(r), std::move(s), proto, M, P, H, fused, true);
            else dev::oversampled_channelizer(std::move(r), std::move(s), proto, M, P, H, fused, true);
        });
        std::thread c = spawn([&, r = std::move(r2)]() mutable { sink(std::move(r), &got, &msgs, &after_first); });
        a.join(); b.join(); c.join();
    }
    dev::set_default_ring_depth(4);
    int route = -1;
    const std::vector<cf> want = bare(mode, proto, M, P, H, fused, data, lens, total, &route);
    const bool equal = want.size() == got.size() && (got.empty() || std::memcmp(want.data(), got.data(), got.size() * sizeof(cf)) == 0);
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    std::fwrite(got.data(), sizeof(cf), got.size(), f);
    std::fclose(f);
    std::printf("%s %zu route %d msgs %zu samples %zu bare_equal %d mallocs_after_first %llu\n", mode.c_str(), depth, route, msgs, got.size(), equal ? 1 : 0,
                after_first);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if ((mode == "stream" || mode == "blocks") && argc == 10)
            return run(mode, (size_t)std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), (size_t)std::atol(argv[5]), std::atoi(argv[6]) != 0, argv[7],
                       argv[8], argv[9]);
        std::fprintf(stderr, "usage: kpn_pfb_os_p2_tests stream|blocks depth nchan taps_per_branch hop fused proto.f32 input.cf32 out.bin\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
