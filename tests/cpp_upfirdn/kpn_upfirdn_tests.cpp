// kpn_upfirdn_tests.cpp -- the rational resampler's blocks of include/kpn_dev.hpp in a device-resident graph, against the bare
// redio_upfirdn_* calls.
//   kpn_upfirdn_tests stream|blocks <depth> <f32|cf32> <up> <down> <fused> <taps.f32> <input> <out.bin>
//       source (the file's samples, uploaded message by message) -> dev::upfirdn_stream / dev::upfirdn -> sink; eight messages of
//       window + 40 period_in + 101 and window + 40 period_in - 37 samples in turn.
// Rings of <depth> buffers; the sink's samples go to <out.bin> in arrival order.  The bare calls: `blocks` is one redio_upfirdn_enqueue
// per message, `stream` is ONE call on the whole input, of which the stream blocks give the whole periods.
// stdout: "<mode> <depth> msgs <n> samples <n> bare_equal <0|1> mallocs_after_first <n>".
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace kpn;

template <typename T>
static void source(Sender<dev::View<T>> v, const std::vector<T> &data, const std::vector<size_t> &lens)
{
    dev::BlockStream st;
    dev::Ring ring;
    size_t first = 0;
    for (size_t len : lens) {
        auto d = ring.acquire<T>(len, st);
        dev::check(redio_upload(d.data(), data.data() + first, len * sizeof(T), st));
        dev::publish(d, st);
        v.send_unwrap(std::move(d));
        first += len;
    }
}

template <typename T>
static void sink(Receiver<dev::View<T>> u, std::vector<T> *all, size_t *msgs, unsigned long long *after_first)
{
    dev::BlockStream st;
    std::vector<T> host;
    unsigned long long m1 = 0;
    try {
        for (;;) {
            auto d = u.recv();
            host.resize(d.len);
            {
                dev::Reading<T> in(d, st);
                dev::check(redio_download(host.data(), d.data(), d.len * sizeof(T), st));
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

template <typename T>
static redio_upfirdn *plan_of(const std::vector<float> &taps, size_t U, size_t D, bool fused)
{
    redio_upfirdn *h = nullptr;
    dev::check(redio_upfirdn_create(&h, taps.data(), taps.size(), U, D, (sizeof(T) == 8 ? REDIO_FIR_COMPLEX : 0) | (fused ? REDIO_FIR_FUSED : 0)));
    return h;
}

// what the bare calls give: per message, or the whole periods of one call on the whole stream
template <typename T>
static std::vector<T> bare(bool stream, redio_upfirdn *h, const std::vector<T> &data, const std::vector<size_t> &lens, size_t total)
{
    void *d_in = nullptr, *d_out = nullptr, *st = nullptr;
    dev::check(redio_stream_create(&st));
    dev::check(redio_malloc(&d_in, total * sizeof(T)));
    dev::check(redio_malloc(&d_out, (redio_upfirdn_nout(h, total) + 1) * sizeof(T)));
    dev::check(redio_upload(d_in, data.data(), total * sizeof(T), st));
    std::vector<T> out;
    auto one = [&](size_t first, size_t len) {
        const size_t n = redio_upfirdn_nout(h, len);
        dev::check(redio_upfirdn_enqueue(h, (const char *)d_in + first * sizeof(T), len, d_out, st));
        const size_t at = out.size();
        out.resize(at + n);
        dev::check(redio_download(out.data() + at, d_out, n * sizeof(T), st));
        dev::check(redio_stream_sync(st));
    };
    if (stream) {
        one(0, total);
        const size_t W = redio_upfirdn_window(h), H = redio_upfirdn_period_in(h);
        out.resize(total < W ? 0 : ((total - W) / H + 1) * redio_upfirdn_period_out(h));
    } else {
        size_t first = 0;
        for (size_t len : lens) { one(first, len); first += len; }
    }
    redio_free(d_in); redio_free(d_out); redio_stream_destroy(st);
    return out;
}

template <typename T>
static int run(const std::string &mode, size_t depth, size_t U, size_t D, bool fused, const std::string &taps_path, const std::string &in_path, const char *path)
{
    const std::vector<float> taps = read_all<float>(taps_path);
    const std::vector<T> data = read_all<T>(in_path);
    const bool stream = mode == "stream";
    redio_upfirdn *h = plan_of<T>(taps, U, D, fused);
    const size_t W = redio_upfirdn_window(h), H = redio_upfirdn_period_in(h);
    std::vector<size_t> lens;
    size_t total = 0;
    for (int i = 0; i < 8; ++i) lens.push_back(W + 40 * H + (i % 2 ? 0 : 101) - (i % 2 ? 37 : 0));
    for (size_t len : lens) total += len;
    if (data.size() < total) { std::fprintf(stderr, "the input file needs %zu samples\n", total); return 1; }
    dev::set_default_ring_depth(depth);
    size_t msgs = 0;
    unsigned long long after_first = 0;
    std::vector<T> got;
    {
        auto [s1, r1] = bounded_channel<dev::View<T>>(8);
        auto [s2, r2] = channel<dev::View<T>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source<T>(std::move(s), data, lens); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
            if (stream) dev::upfirdn_stream<T>(std::move(r), std::move(s), taps, U, D, fused);
            else dev::upfirdn<T>(std::move(r), std::move(s), taps, U, D, fused);
        });
        std::thread c = spawn([&, r = std::move(r2)]() mutable { sink<T>(std::move(r), &got, &msgs, &after_first); });
        a.join(); b.join(); c.join();
    }
    dev::set_default_ring_depth(4);
    const std::vector<T> want = bare<T>(stream, h, data, lens, total);
    redio_upfirdn_destroy(h);
    const bool equal = want.size() == got.size() && (got.empty() || std::memcmp(want.data(), got.data(), got.size() * sizeof(T)) == 0);
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    std::fwrite(got.data(), sizeof(T), got.size(), f);
    std::fclose(f);
    std::printf("%s %zu msgs %zu samples %zu bare_equal %d mallocs_after_first %llu\n", mode.c_str(), depth, msgs, got.size(), equal ? 1 : 0, after_first);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "", kind = argc > 3 ? argv[3] : "";
        if ((mode == "stream" || mode == "blocks") && (kind == "f32" || kind == "cf32") && argc == 10) {
            const size_t depth = (size_t)std::atoi(argv[2]), U = (size_t)std::atol(argv[4]), D = (size_t)std::atol(argv[5]);
            const bool fused = std::atoi(argv[6]) != 0;
            if (kind == "f32") return run<float>(mode, depth, U, D, fused, argv[7], argv[8], argv[9]);
            return run<std::complex<float>>(mode, depth, U, D, fused, argv[7], argv[8], argv[9]);
        }
        std::fprintf(stderr, "usage: kpn_upfirdn_tests stream|blocks depth f32|cf32 up down fused taps.f32 input out.bin\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
