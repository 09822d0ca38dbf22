// kpn_ddc_upfirdn_tests.cpp -- the tuned resampler's blocks of include/kpn_dev.hpp in a device-resident graph, against the bare
// redio_ddc_upfirdn_* calls.
//   kpn_ddc_upfirdn_tests stream|blocks <depth> <cf32|u8> <up> <down> <fused> <osc.c32> <taps.f32> <input> <out.bin>
//       source (the file's samples, uploaded message by message) -> dev::tuned_resampler_stream[_u8] / dev::tuned_resampler[_u8] -> sink;
//       eight messages of ntaps + 40 down + 101 and ntaps + 40 down - 37 samples in turn.
// <input>: cf32 samples, or with u8 interleaved I/Q bytes, two per sample.  Rings of <depth> buffers; the sink's cf32 samples go to
// <out.bin> in arrival order.  The bare calls: `blocks` is one redio_ddc_upfirdn_enqueue[_u8] per message with first_index 0 (the
// per-message blocks restart the table and the phase), `stream` is ONE call on the whole input with first_index 0, cut to the whole
// periods the stream blocks emit (they carry phase and history).
// stdout: "<mode> <depth> msgs <n> samples <n> bare_equal <0|1> mallocs_after_first <n>".
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace kpn;
using cf = std::complex<float>;

template <typename T>
static void source(Sender<dev::View<T>> v, const std::vector<T> &data, const std::vector<size_t> &lens, size_t E)
{
    dev::BlockStream st;
    dev::Ring ring;
    size_t first = 0;
    for (size_t len : lens) {
        auto d = ring.acquire<T>(E * len, st);
        dev::check(redio_upload(d.data(), data.data() + E * first, E * len * sizeof(T), st));
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

// what the bare calls give: per message with first_index 0, or one call on the whole stream
template <typename T>
static std::vector<cf> bare(bool stream, const std::vector<cf> &osc, const std::vector<float> &taps, size_t U, size_t D, bool fused, const std::vector<T> &data,
                            const std::vector<size_t> &lens, size_t total, size_t E)
{
    redio_ddc_upfirdn *h = nullptr;
    dev::check(redio_ddc_upfirdn_create(&h, reinterpret_cast<const float *>(osc.data()), osc.size(), taps.data(), taps.size(), U, D, fused ? REDIO_FIR_FUSED : 0));
    void *d_in = nullptr, *d_out = nullptr, *st = nullptr;
    dev::check(redio_stream_create(&st));
    dev::check(redio_malloc(&d_in, E * total * sizeof(T)));
    dev::check(redio_malloc(&d_out, (redio_ddc_upfirdn_nout(h, total) + 1) * sizeof(cf)));
    dev::check(redio_upload(d_in, data.data(), E * total * sizeof(T), st));
    std::vector<cf> out;
    auto one = [&](size_t first, size_t len) {
        const size_t n = redio_ddc_upfirdn_nout(h, len);
        const char *in = (const char *)d_in + E * first * sizeof(T);
        if (sizeof(T) == 1) dev::check(redio_ddc_upfirdn_enqueue_u8(h, in, 2 * len, 0, d_out, st));
        else dev::check(redio_ddc_upfirdn_enqueue(h, in, len, 0, d_out, st));
        const size_t at = out.size();
        out.resize(at + n);
        dev::check(redio_download(out.data() + at, d_out, n * sizeof(cf), st));
        dev::check(redio_stream_sync(st));
    };
    if (stream) {
        one(0, total);
        const size_t Up = redio_ddc_upfirdn_period_out(h), Dp = redio_ddc_upfirdn_period_in(h), Wp = redio_ddc_upfirdn_window(h);
        out.resize(total < Wp ? 0 : Up * ((total - Wp) / Dp + 1)); // whole periods
    } else {
        size_t first = 0;
        for (size_t len : lens) { one(first, len); first += len; }
    }
    redio_free(d_in); redio_free(d_out); redio_stream_destroy(st); redio_ddc_upfirdn_destroy(h);
    return out;
}

template <typename T>
static int run(const std::string &mode, size_t depth, size_t U, size_t D, bool fused, const std::string &osc_path, const std::string &taps_path, const std::string &in_path,
               const char *path)
{
    constexpr bool U8 = sizeof(T) == 1;
    const size_t E = U8 ? 2 : 1;
    const std::vector<cf> osc = read_all<cf>(osc_path);
    const std::vector<float> taps = read_all<float>(taps_path);
    const std::vector<T> data = read_all<T>(in_path);
    const bool stream = mode == "stream";
    std::vector<size_t> lens;
    size_t total = 0;
    for (int i = 0; i < 8; ++i) lens.push_back(taps.size() + 40 * D + (i % 2 ? 0 : 101) - (i % 2 ? 37 : 0));
    for (size_t len : lens) total += len;
    if (data.size() < E * total) { std::fprintf(stderr, "the input file needs %zu samples\n", total); return 1; }
    dev::set_default_ring_depth(depth);
    size_t msgs = 0;
    unsigned long long after_first = 0;
    std::vector<cf> got;
    {
        auto [s1, r1] = bounded_channel<dev::View<T>>(8);
        auto [s2, r2] = channel<dev::View<cf>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source<T>(std::move(s), data, lens, E); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
            if constexpr (U8) {
                if (stream) dev::tuned_resampler_stream_u8(std::move(r), std::move(s), osc, taps, U, D, fused);
                else dev::tuned_resampler_u8(std::move(r), std::move(s), osc, taps, U, D, fused);
            } else {
                if (stream) dev::tuned_resampler_stream(std::move(r), std::move(s), osc, taps, U, D, fused);
                else dev::tuned_resampler(std::move(r), std::move(s), osc, taps, U, D, fused);
            }
        });
        std::thread c = spawn([&, r = std::move(r2)]() mutable { sink(std::move(r), &got, &msgs, &after_first); });
        a.join(); b.join(); c.join();
    }
    dev::set_default_ring_depth(4);
    const std::vector<cf> want = bare<T>(stream, osc, taps, U, D, fused, data, lens, total, E);
    const bool equal = want.size() == got.size() && (got.empty() || std::memcmp(want.data(), got.data(), got.size() * sizeof(cf)) == 0);
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    std::fwrite(got.data(), sizeof(cf), got.size(), f);
    std::fclose(f);
    std::printf("%s %zu msgs %zu samples %zu bare_equal %d mallocs_after_first %llu\n", mode.c_str(), depth, msgs, got.size(), equal ? 1 : 0, after_first);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "", kind = argc > 3 ? argv[3] : "";
        if ((mode == "stream" || mode == "blocks") && (kind == "cf32" || kind == "u8") && argc == 11) {
            const size_t depth = (size_t)std::atoi(argv[2]), U = (size_t)std::atol(argv[4]), D = (size_t)std::atol(argv[5]);
            const bool fused = std::atoi(argv[6]) != 0;
            if (kind == "u8") return run<uint8_t>(mode, depth, U, D, fused, argv[7], argv[8], argv[9], argv[10]);
            return run<cf>(mode, depth, U, D, fused, argv[7], argv[8], argv[9], argv[10]);
        }
        std::fprintf(stderr, "usage: kpn_ddc_upfirdn_tests stream|blocks depth cf32|u8 up down fused osc.c32 taps.f32 input out.bin\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
