// kpn_fftr_tests.cpp -- the real-input transform blocks of include/kpn_dev.hpp (dev::fftr, dev::fftri) in a device-resident graph.
//   kpn_fftr_tests round_trip <depth> <out.bin>   synthetic f32 source -> dev::fftr(2048) -> dev::fftri(2048) -> sink, 12 messages of
//                                                 1, 2 and 5 blocks in turn through rings of <depth> buffers; the sink's f32 words go
//                                                 to <out.bin> in arrival order; stdout: "round_trip <depth> msgs <n> words <n>"
//   kpn_fftr_tests short_message                  one message of 2047 samples: the block's assert text on stdout, exit status 0
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace kpn;
using cf = std::complex<float>;

static const uint32_t SEED = 0x5EED0F7Au;
static const uint32_t N = 2048;

static void source(Sender<dev::View<float>> v, const std::vector<size_t> &lens)
{
    dev::BlockStream st;
    dev::Ring ring;
    uint64_t first = 0;
    for (size_t len : lens) {
        auto d = ring.acquire<float>(len, st);
        dev::check(redio_synth_f32(d.data(), SEED, first, len, st));
        dev::publish(d, st);
        v.send_unwrap(std::move(d));
        first += len;
    }
}

static void file_sink(Receiver<dev::View<float>> u, std::FILE *f, size_t *msgs, size_t *words)
{
    dev::BlockStream st;
    std::vector<float> host;
    try {
        for (;;) {
            auto d = u.recv();
            host.resize(d.len);
            {
                dev::Reading<float> in(d, st);
                dev::check(redio_download(host.data(), d.data(), d.len * sizeof(float), st));
            }
            dev::check(redio_stream_sync(st));
            std::fwrite(host.data(), sizeof(float), host.size(), f);
            ++*msgs;
            *words += d.len;
        }
    } catch (const hangup &) {
    }
}

static int round_trip(size_t depth, const char *path)
{
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    dev::set_default_ring_depth(depth);
    std::vector<size_t> lens;
    const size_t blocks[3] = {1, 2, 5};
    for (int i = 0; i < 12; ++i) lens.push_back(blocks[i % 3] * N);
    size_t msgs = 0, words = 0;
    {
        auto [s1, r1] = bounded_channel<dev::View<float>>(8);
        auto [s2, r2] = channel<dev::View<cf>>();
        auto [s3, r3] = channel<dev::View<float>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source(std::move(s), lens); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable { dev::fftr(std::move(r), std::move(s), N); });
        std::thread c = spawn([&, r = std::move(r2), s = std::move(s3)]() mutable { dev::fftri(std::move(r), std::move(s), N); });
        std::thread d = spawn([&, r = std::move(r3)]() mutable { file_sink(std::move(r), f, &msgs, &words); });
        a.join(); b.join(); c.join(); d.join();
    }
    std::fclose(f);
    dev::set_default_ring_depth(4);
    std::printf("round_trip %zu msgs %zu words %zu\n", depth, msgs, words);
    return 0;
}

static int short_message()
{
    std::string what = "no exception";
    auto [s1, r1] = channel<dev::View<float>>();
    auto [s2, r2] = channel<dev::View<cf>>();
    std::thread a = spawn([&, s = std::move(s1)]() mutable { source(std::move(s), {N - 1}); });
    std::thread b([&, r = std::move(r1), s = std::move(s2)]() mutable {
        try {
            dev::fftr(std::move(r), std::move(s), N);
        } catch (const hangup &) {
            what = "hangup";
        } catch (const std::exception &e) {
            what = e.what();
        }
    });
    a.join(); b.join();
    std::printf("short_message %s\n", what.c_str());
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "round_trip" && argc == 4) return round_trip((size_t)std::atoi(argv[2]), argv[3]);
        if (mode == "short_message") return short_message();
        std::fprintf(stderr, "usage: kpn_fftr_tests round_trip depth out.bin | short_message\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
