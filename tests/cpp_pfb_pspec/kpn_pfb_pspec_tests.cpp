// kpn_pfb_pspec_tests.cpp -- the polyphase spectrometer blocks of include/kpn_dev.hpp in a device-resident graph.
//   kpn_pfb_pspec_tests stream <depth> <cf32|u8> <nchan> <taps_per_branch> <integrate> <proto.f32> <input> <out.bin>
//       source (the file's samples, uploaded message by message) -> dev::polyphase_spectrum_stream[_u8] -> sink; with
//       W = (integrate - 1 + taps_per_branch) nchan and H = integrate nchan the messages hold W + 2 H samples, then 2 H - 100 and
//       2 H + 100 in turn (ten of them): 3, then 1 and 3 rows
//   kpn_pfb_pspec_tests blocks ...
//       the same source -> dev::polyphase_spectrum[_u8] -> sink, 12 messages that hold exactly 3, 1 and 2 rows in turn
// <input>: cf32 samples, or with u8 interleaved I/Q bytes, two per sample.  Rings of <depth> buffers; the sink's f32 words go to
// <out.bin> in arrival order; stdout: "<mode> <depth> msgs <n> words <n> mallocs_after_first <n>" (redio_malloc_count() from the
// sink's first message to the end).
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>

using namespace kpn;

// message i holds lens[i] samples of E elements each
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
static int run(const std::string &mode, size_t depth, int M, int P, size_t K, const std::string &proto_path, const std::string &in_path, const char *path)
{
    constexpr bool U8 = sizeof(T) == 1;
    const size_t E = U8 ? 2 : 1;
    const std::vector<float> proto = read_all<float>(proto_path);
    if (proto.size() != (size_t)M * (size_t)P) { std::fprintf(stderr, "the prototype needs %d taps\n", M * P); return 1; }
    const std::vector<T> data = read_all<T>(in_path);
    const size_t W = (K - 1 + (size_t)P) * (size_t)M, H = K * (size_t)M;
    std::vector<size_t> lens;
    size_t total = 0;
    if (mode == "stream") {
        if (H <= 100) { std::fprintf(stderr, "integrate * nchan must exceed 100\n"); return 1; }
        lens.push_back(W + 2 * H);
        for (int i = 0; i < 10; ++i) lens.push_back(i % 2 ? 2 * H + 100 : 2 * H - 100);
    } else {
        const size_t rows[3] = {3, 1, 2};
        for (int i = 0; i < 12; ++i) lens.push_back(W + (rows[i % 3] - 1) * H);
    }
    for (size_t len : lens) total += len;
    if (data.size() < E * total) { std::fprintf(stderr, "the input file needs %zu samples\n", total); return 1; }
    std::FILE *f = std::fopen(path, "wb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 1; }
    dev::set_default_ring_depth(depth);
    size_t msgs = 0, words = 0;
    unsigned long long after_first = 0;
    {
        auto [s1, r1] = bounded_channel<dev::View<T>>(8);
        auto [s2, r2] = channel<dev::View<float>>();
        std::thread a = spawn([&, s = std::move(s1)]() mutable { source<T>(std::move(s), data, lens, E); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
            if constexpr (U8) {
                if (mode == "stream") dev::polyphase_spectrum_stream_u8(std::move(r), std::move(s), proto, M, P, K);
                else dev::polyphase_spectrum_u8(std::move(r), std::move(s), proto, M, P, K);
            } else {
                if (mode == "stream") dev::polyphase_spectrum_stream(std::move(r), std::move(s), proto, M, P, K);
                else dev::polyphase_spectrum(std::move(r), std::move(s), proto, M, P, K);
            }
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
        const std::string mode = argc > 1 ? argv[1] : "", kind = argc > 3 ? argv[3] : "";
        if ((mode == "stream" || mode == "blocks") && (kind == "cf32" || kind == "u8") && argc == 10) {
            const size_t depth = (size_t)std::atoi(argv[2]);
            const int M = std::atoi(argv[4]), P = std::atoi(argv[5]);
            const size_t K = (size_t)std::atol(argv[6]);
            if (kind == "u8") return run<uint8_t>(mode, depth, M, P, K, argv[7], argv[8], argv[9]);
            return run<std::complex<float>>(mode, depth, M, P, K, argv[7], argv[8], argv[9]);
        }
        std::fprintf(stderr, "usage: kpn_pfb_pspec_tests stream|blocks depth cf32|u8 nchan taps_per_branch integrate proto.f32 input out.bin\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
