// kpn_ovsave_real_tests.cpp -- the real overlap-save blocks of include/kpn_dev.hpp in a device-resident graph.
//   kpn_ovsave_real_tests stream <depth> <taps.f32> <out.bin>   synthetic f32 source -> dev::overlap_save_real_stream(taps, 2048) -> sink,
//                                                                12 messages of uneven lengths (odd ones among them)
//   kpn_ovsave_real_tests blocks <depth> <taps.f32> <out.bin>   the same source -> dev::overlap_save_real(taps, 2048) -> sink, 12 messages
//                                                                that hold exactly 1, 2 and 5 blocks in turn
// Rings of <depth> buffers; the sink's f32 words go to <out.bin> in arrival order; stdout: "<mode> <depth> msgs <n> words <n>".
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace kpn;

static const uint32_t SEED = 0x5EED0A5Eu;
static const int N = 2048;

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

static std::vector<float> read_taps(const char *path)
{
    std::vector<float> t;
    std::FILE *f = std::fopen(path, "rb");
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    float v;
    while (std::fread(&v, sizeof v, 1, f) == 1) t.push_back(v);
    std::fclose(f);
    return t;
}

static int run(const std::string &mode, size_t depth, const char *taps_path, const char *path)
{
    const std::vector<float> taps = read_taps(taps_path);
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    dev::set_default_ring_depth(depth);
    std::vector<size_t> lens;
    if (mode == "stream") {
        lens = {1, 7, 1921, 1922, 2048, 2049, 6149, 333, 4097, 1000, 5001, 12345};
    } else {
        const size_t hop = (size_t)N - (taps.size() | 1) + 1, blocks[3] = {1, 2, 5};
        for (int i = 0; i < 12; ++i) lens.push_back((size_t)N + (blocks[i % 3] - 1) * hop);
    }
    size_t msgs = 0, words = 0;
    {
        auto [s1, r1] = bounded_channel<dev::View<float>>(8);
        auto [s2, r2] = channel<dev::View<float>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source(std::move(s), lens); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
            if (mode == "stream") dev::overlap_save_real_stream(std::move(r), std::move(s), taps, N);
            else dev::overlap_save_real(std::move(r), std::move(s), taps, N);
        });
        std::thread c = spawn([&, r = std::move(r2)]() mutable { file_sink(std::move(r), f, &msgs, &words); });
        a.join(); b.join(); c.join();
    }
    std::fclose(f);
    dev::set_default_ring_depth(4);
    std::printf("%s %zu msgs %zu words %zu\n", mode.c_str(), depth, msgs, words);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if ((mode == "stream" || mode == "blocks") && argc == 5) return run(mode, (size_t)std::atoi(argv[2]), argv[3], argv[4]);
        std::fprintf(stderr, "usage: kpn_ovsave_real_tests stream|blocks depth taps.f32 out.bin\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
