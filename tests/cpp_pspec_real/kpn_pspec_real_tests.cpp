// kpn_pspec_real_tests.cpp -- the real-input power-spectrum blocks of include/kpn_dev.hpp in a device-resident graph.
//   kpn_pspec_real_tests stream <depth> <nfft> <integrate> <step> <window.f32|none> <out.bin>
//       synthetic f32 source -> dev::power_spectrum_real_stream -> sink; with W = (integrate - 1) step + nfft and H = integrate step the
//       messages hold W + 2 H samples, then 2 H - 100 and 2 H + 100 in turn (ten of them): 3, then 1 and 3 rows
//   kpn_pspec_real_tests blocks <depth> <nfft> <integrate> <step> <window.f32|none> <out.bin>
//       the same source -> dev::power_spectrum_real -> sink, 12 messages that hold exactly 3, 1 and 2 rows in turn
// Rings of <depth> buffers; the sink's f32 words go to <out.bin> in arrival order; stdout:
// "<mode> <depth> msgs <n> words <n> mallocs_after_first <n>" (redio_malloc_count() from the sink's first message to the end).
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace kpn;

static const uint32_t SEED = 0x5EED0B5Du;

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

static void file_sink(Receiver<dev::View<float>> u, std::FILE *f, size_t *msgs, size_t *words, unsigned long long *after_first)
{
    dev::BlockStream st;
    std::vector<float> host;
    unsigned long long m1 = 0;
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
            if (++*msgs == 1) m1 = redio_malloc_count();
            *words += d.len;
        }
    } catch (const hangup &) {
    }
    *after_first = redio_malloc_count() - m1;
}

static std::vector<float> read_f32(const std::string &path)
{
    std::vector<float> t;
    if (path == "none") return t;
    std::FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot open " + path);
    float v;
    while (std::fread(&v, sizeof v, 1, f) == 1) t.push_back(v);
    std::fclose(f);
    return t;
}

static int run(const std::string &mode, size_t depth, int nfft, size_t K, size_t step, const std::string &win_path, const char *path)
{
    const std::vector<float> win = read_f32(win_path);
    if (!win.empty() && win.size() != (size_t)nfft) { std::fprintf(stderr, "the window needs %d values\n", nfft); return 1; }
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    dev::set_default_ring_depth(depth);
    const size_t W = (K - 1) * step + (size_t)nfft, H = K * step;
    std::vector<size_t> lens;
    if (mode == "stream") {
        if (H <= 100) { std::fprintf(stderr, "integrate * step must exceed 100\n"); return 1; }
        lens.push_back(W + 2 * H);
        for (int i = 0; i < 10; ++i) lens.push_back(i % 2 ? 2 * H + 100 : 2 * H - 100);
    } else {
        const size_t rows[3] = {3, 1, 2};
        for (int i = 0; i < 12; ++i) lens.push_back(W + (rows[i % 3] - 1) * H);
    }
    size_t msgs = 0, words = 0;
    unsigned long long after_first = 0;
    {
        auto [s1, r1] = bounded_channel<dev::View<float>>(8);
        auto [s2, r2] = channel<dev::View<float>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source(std::move(s), lens); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
            if (mode == "stream") dev::power_spectrum_real_stream(std::move(r), std::move(s), nfft, K, step, win);
            else dev::power_spectrum_real(std::move(r), std::move(s), nfft, K, step, win);
        });
        std::thread c = spawn([&, r = std::move(r2)]() mutable { file_sink(std::move(r), f, &msgs, &words, &after_first); });
        a.join(); b.join(); c.join();
    }
    std::fclose(f);
    dev::set_default_ring_depth(4);
    std::printf("%s %zu msgs %zu words %zu mallocs_after_first %llu\n", mode.c_str(), depth, msgs, words, after_first);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if ((mode == "stream" || mode == "blocks") && argc == 8)
            return run(mode, (size_t)std::atoi(argv[2]), std::atoi(argv[3]), (size_t)std::atol(argv[4]), (size_t)std::atol(argv[5]), argv[6], argv[7]);
        std::fprintf(stderr, "usage: kpn_pspec_real_tests stream|blocks depth nfft integrate step window.f32|none out.bin\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
