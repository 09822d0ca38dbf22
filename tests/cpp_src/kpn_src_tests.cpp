// kpn_src_tests.cpp -- the queue-ordered resampler call (redio_src_enqueue) and the blocks built on it and on the layout kernels
// (include/kpn_dev.hpp: dev::resample_channels, dev::channel_planes, dev::plane_rows).
//   kpn_src_tests src_gpu                 synthetic f32 source -> dev::resample_channels(64, 0.02) -> checksum sink, 40 messages of
//                                         64 x 4096 frames, under both stream policies and ring depths (default, 1), against the same
//                                         calls made bare through redio_src_process: one line
//                                         "src_gpu <policy> <depth> graph <sum> <msgs> bare <sum> <msgs> lens_equal <0|1> mallocs_after_2 <n>
//                                          queued <n> synchronised <n>" per setting
//   kpn_src_tests c4c3                    synth_iq -> channelizer(64, 16) -> channel_planes(64) -> resample_channels(128, 0.5) ->
//                                         plane_rows(64) -> checksum sink against the same calls made bare: "c4c3 graph ... bare ..."
//   kpn_src_tests bench nch log2f mode    one JSON line: us per message of bare redio_src_process, bare redio_src_enqueue with one
//                                         synchronisation at the end, and the dev::resample_channels graph with a drop sink
//   kpn_src_tests bench_planes log2r nch  one JSON line: the layout kernels both ways against redio_copy of the same bytes
#include "../../include/kpn.hpp"
#include "../../include/kpn_dev.hpp"
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

using namespace kpn;
using cf = std::complex<float>;
using clk = std::chrono::steady_clock;
static double secs(clk::time_point a, clk::time_point b) { return std::chrono::duration<double>(b - a).count(); }

struct Run {
    unsigned long long sum = 0, mallocs_after_2 = 0;
    std::vector<size_t> lens;
    long counts[2] = {0, 0}; // queued, synchronised
};

// checksum sink that also keeps every message's length and the device allocation count from the second message on
template <typename T>
static void recording_sink(Receiver<dev::View<T>> u, Run *run)
{
    dev::BlockStream st;
    auto acc = dev::make<unsigned long long>(1);
    const unsigned long long zero = 0;
    dev::check(redio_upload(acc.data(), &zero, sizeof(zero), st));
    dev::check(redio_stream_sync(st));
    unsigned long long m2 = 0;
    try {
        for (;;) {
            auto d = u.recv();
            dev::Reading<T> in(d, st);
            dev::check(redio_checksum_u32(d.data(), d.len * sizeof(T) / 4, acc.data(), st));
            run->lens.push_back(d.len);
            if (run->lens.size() == 2) m2 = redio_malloc_count();
        }
    } catch (const hangup &) {
    }
    dev::check(redio_download(&run->sum, acc.data(), sizeof(run->sum), st));
    dev::check(redio_stream_sync(st));
    run->mallocs_after_2 = redio_malloc_count() - m2;
}

static void synth_f32_source(Sender<dev::View<float>> v, uint32_t seed, size_t msg_len, size_t nmsg)
{
    dev::BlockStream st;
    dev::Ring ring;
    for (size_t i = 0; i < nmsg; ++i) {
        auto d = ring.acquire<float>(msg_len, st);
        dev::check(redio_synth_f32(d.data(), seed, (uint64_t)i * msg_len, msg_len, st));
        dev::publish(d, st);
        v.send_unwrap(std::move(d));
    }
}

static int src_gpu()
{
    const int nch = 64;
    const size_t frames = 4096, nmsg = 40, msg = (size_t)nch * frames;
    const double ratio = 0.02;
    const uint32_t seed = 0x5EED0003u;
    // bare: the same messages through redio_src_process, rows at stride lout, every row's gen samples into the checksum
    Run bare;
    {
        void *st = nullptr;
        dev::check(redio_stream_create(&st));
        const long lout = (long)(ratio * (double)frames + 1.0);
        auto x = dev::make<float>(msg), y = dev::make<float>((size_t)lout * nch);
        auto acc = dev::make<unsigned long long>(1);
        const unsigned long long zero = 0;
        dev::check(redio_upload(acc.data(), &zero, 8, st));
        redio_src *h = nullptr;
        dev::check(redio_src_create(&h, 1, nch));
        for (size_t i = 0; i < nmsg; ++i) {
            dev::check(redio_synth_f32(x.data(), seed, (uint64_t)i * msg, msg, st));
            long used = 0, gen = 0;
            dev::check(redio_src_process(h, x.data(), (long)frames, (long)frames, y.data(), lout, lout, ratio, 0, &used, &gen, st));
            for (int c = 0; c < nch; ++c) dev::check(redio_checksum_u32(y.data() + (size_t)c * lout, (size_t)gen, acc.data(), st));
            bare.lens.push_back((size_t)gen * nch);
        }
        dev::check(redio_download(&bare.sum, acc.data(), 8, st));
        dev::check(redio_stream_sync(st));
        redio_src_destroy(h);
        redio_stream_destroy(st);
    }
    for (int policy = 0; policy < 2; ++policy)
        for (size_t depth : {(size_t)4, (size_t)1}) {
            dev::set_stream_policy(policy ? dev::PER_BLOCK : dev::SHARED);
            dev::set_default_ring_depth(depth);
            Run g;
            {
                auto [s1, r1] = bounded_channel<dev::View<float>>(8);
                auto [s2, r2] = channel<dev::View<float>>();
                std::thread a = spawn([&, s = std::move(s1)]() mutable { synth_f32_source(std::move(s), seed, msg, nmsg); });
                std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable {
                    dev::resample_channels(std::move(r), std::move(s), nch, ratio, 1, REDIO_SRC_EXACT, g.counts);
                });
                std::thread c = spawn([&, r = std::move(r2)]() mutable { recording_sink<float>(std::move(r), &g); });
                a.join(); b.join(); c.join();
            }
            std::printf("src_gpu %s %zu graph %llu %zu bare %llu %zu lens_equal %d mallocs_after_2 %llu queued %ld synchronised %ld\n",
                        policy ? "per_block" : "shared", depth, g.sum, g.lens.size(), bare.sum, bare.lens.size(), (int)(g.lens == bare.lens),
                        g.mallocs_after_2, g.counts[0], g.counts[1]);
        }
    dev::set_stream_policy(dev::SHARED);
    dev::set_default_ring_depth(4);
    return 0;
}

static int c4c3()
{
    const int M = 64, P = 16;
    const size_t rows = 1024, n_in = (size_t)M * (rows + P - 1), nmsg = 12;
    const double ratio = 0.5;
    const uint32_t seed = 0x5EED0004u;
    const std::vector<float> proto = dsputils::lpf_corrected((size_t)M * P, 0.45f / M);
    Run bare;
    {
        void *st = nullptr;
        dev::check(redio_stream_create(&st));
        redio_pfb *pfb = nullptr;
        dev::check(redio_pfb_create(&pfb, proto.data(), M, P, REDIO_FIR_FUSED));
        if (redio_pfb_nrows(pfb, n_in) != rows) { std::fprintf(stderr, "c4c3: unexpected row count\n"); return 1; }
        redio_src *h = nullptr;
        dev::check(redio_src_create(&h, 1, 2 * M));
        const long lout = (long)(ratio * (double)rows + 1.0);
        auto x = dev::make<cf>(n_in), r = dev::make<cf>(rows * M), back = dev::make<cf>((size_t)lout * M);
        auto pl = dev::make<float>(2 * M * rows), y = dev::make<float>((size_t)2 * M * lout);
        auto acc = dev::make<unsigned long long>(1);
        const unsigned long long zero = 0;
        dev::check(redio_upload(acc.data(), &zero, 8, st));
        for (size_t i = 0; i < nmsg; ++i) {
            dev::check(redio_synth_iq(x.data(), seed, (uint64_t)i * n_in, n_in, st));
            dev::check(redio_pfb_enqueue(pfb, x.data(), n_in, r.data(), 1, st));
            dev::check(redio_rows_to_planes_c32(r.data(), rows, M, pl.data(), rows, st));
            long used = 0, gen = 0;
            dev::check(redio_src_process(h, pl.data(), (long)rows, (long)rows, y.data(), lout, lout, ratio, 0, &used, &gen, st));
            dev::check(redio_planes_to_rows_c32(y.data(), (size_t)lout, (size_t)gen, M, back.data(), st));
            dev::check(redio_checksum_u32(back.data(), (size_t)gen * M * 2, acc.data(), st));
            bare.lens.push_back((size_t)gen * M);
        }
        dev::check(redio_download(&bare.sum, acc.data(), 8, st));
        dev::check(redio_stream_sync(st));
        redio_src_destroy(h);
        redio_pfb_destroy(pfb);
        redio_stream_destroy(st);
    }
    Run g;
    {
        auto [s1, r1] = bounded_channel<dev::View<cf>>(8);
        auto [s2, r2] = channel<dev::View<cf>>();
        auto [s3, r3] = channel<dev::View<float>>();
        auto [s4, r4] = channel<dev::View<float>>();
        auto [s5, r5] = channel<dev::View<cf>>();
        std::vector<std::thread> th;
        th.push_back(spawn([&, s = std::move(s1)]() mutable { dev::synth_iq_source(std::move(s), seed, n_in, nmsg); }));
        th.push_back(spawn([&, r = std::move(r1), s = std::move(s2)]() mutable { dev::channelizer(std::move(r), std::move(s), proto, M, P, true); }));
        th.push_back(spawn([&, r = std::move(r2), s = std::move(s3)]() mutable { dev::channel_planes(std::move(r), std::move(s), M); }));
        th.push_back(spawn([&, r = std::move(r3), s = std::move(s4)]() mutable {
            dev::resample_channels(std::move(r), std::move(s), 2 * M, ratio, 1, REDIO_SRC_EXACT, g.counts);
        }));
        th.push_back(spawn([&, r = std::move(r4), s = std::move(s5)]() mutable { dev::plane_rows(std::move(r), std::move(s), M); }));
        th.push_back(spawn([&, r = std::move(r5)]() mutable { recording_sink<cf>(std::move(r), &g); }));
        for (auto &t : th) t.join();
    }
    std::printf("c4c3 graph %llu %zu bare %llu %zu lens_equal %d queued %ld synchronised %ld\n", g.sum, g.lens.size(), bare.sum, bare.lens.size(),
                (int)(g.lens == bare.lens), g.counts[0], g.counts[1]);
    return 0;
}

// ---- bench ----
static int bench(int nch, int log2f, const std::string &mode_name)
{
    if (nch < 1 || nch > 4096 || log2f < 8 || log2f > 24 || (mode_name != "exact" && mode_name != "fast")) {
        std::fprintf(stderr, "bench: 1 <= nch <= 4096, 8 <= log2_frames <= 24, exact | fast\n");
        return 2;
    }
    const int mode = mode_name == "fast" ? REDIO_SRC_FAST : REDIO_SRC_EXACT;
    const size_t frames = (size_t)1 << log2f, msg = (size_t)nch * frames, R = msg * 4 > ((size_t)2 << 30) ? 2 : 4;
    const double ratio = 0.02;
    const long lout = (long)(ratio * (double)frames + 1.0);
    auto big = dev::make<float>(R * msg);
    dev::check(redio_synth_f32(big.data(), 0x5EED0003u, 0, R * msg, nullptr));
    dev::check(redio_stream_sync(nullptr));
    auto outs = dev::make<float>(4 * (size_t)lout * nch);
    dev::BlockStream st(dev::BlockStream::TRANSFER);
    redio_src *hp = nullptr, *he = nullptr;
    dev::check(redio_src_create(&hp, 1, nch)); dev::check(redio_src_set_mode(hp, mode));
    dev::check(redio_src_create(&he, 1, nch)); dev::check(redio_src_set_mode(he, mode));
    auto process = [&](size_t n) {
        long u = 0, g = 0;
        for (size_t i = 0; i < n; ++i)
            dev::check(redio_src_process(hp, big.data() + (i % R) * msg, (long)frames, (long)frames, outs.data() + (i % 4) * (size_t)lout * nch, lout, lout, ratio, 0, &u, &g, st));
    };
    auto enqueue = [&](size_t n) {
        long u = 0, g = 0;
        for (size_t i = 0; i < n; ++i)
            dev::check(redio_src_enqueue(he, big.data() + (i % R) * msg, (long)frames, (long)frames, outs.data() + (i % 4) * (size_t)lout * nch, lout, 0, ratio, &u, &g, st));
        dev::check(redio_stream_sync(st));
    };
    process(4); enqueue(4);
    auto t0 = clk::now();
    size_t done = 0;
    while (secs(t0, clk::now()) < 0.1) { process(4); done += 4; }
    const double per = secs(t0, clk::now()) / (double)done;
    const size_t nmsg = std::max<size_t>(8, (size_t)(0.25 / per));
    double bare_process = 1e30, bare_enqueue = 1e30;
    for (int rep = 0; rep < 3; ++rep) { // interleaved, best of three
        auto a = clk::now(); process(nmsg); auto b = clk::now(); enqueue(nmsg); auto c = clk::now();
        bare_process = std::min(bare_process, secs(a, b) / (double)nmsg * 1e6);
        bare_enqueue = std::min(bare_enqueue, secs(b, c) / (double)nmsg * 1e6);
    }
    long q = 0, sy = 0;
    redio_src_enqueue_counts(he, &q, &sy);
    redio_src_destroy(hp); redio_src_destroy(he);
    // the graph: resident source -> dev::resample_channels -> drop sink; the host clock between two completed synchronisations
    const size_t warm = std::max<size_t>(8, (size_t)(0.05 / per)), gn = nmsg, total = warm + gn;
    double graph_us = 1e30;
    unsigned long long mallocs = 0;
    for (int rep = 0; rep < 2; ++rep) {
        auto [s1, r1] = bounded_channel<dev::View<float>>(8);
        auto [s2, r2] = channel<dev::View<float>>();
        clk::time_point g0, g1;
        unsigned long long m0 = 0, m1 = 0;
        std::thread a = spawn([&, s = std::move(s1)]() mutable { for (size_t i = 0; i < total; ++i) s.send_unwrap(big.sub((i % R) * msg, msg)); });
        std::thread b = spawn([&, r = std::move(r1), s = std::move(s2)]() mutable { dev::resample_channels(std::move(r), std::move(s), nch, ratio, 1, mode); });
        std::thread c = spawn([&, r = std::move(r2)]() mutable {
            dev::BlockStream sst;
            for (size_t i = 0; i < total; ++i) {
                auto d = r.recv();
                { dev::Reading<float> in(d, sst); }
                d = dev::View<float>();
                if (i + 1 == warm) { dev::check(redio_stream_sync(sst)); m0 = redio_malloc_count(); g0 = clk::now(); }
            }
            dev::check(redio_stream_sync(sst));
            g1 = clk::now();
            m1 = redio_malloc_count();
        });
        a.join(); b.join(); c.join();
        graph_us = std::min(graph_us, secs(g0, g1) / (double)gn * 1e6);
        mallocs += m1 - m0;
    }
    std::printf("{\"mode\": \"bench\", \"nch\": %d, \"log2_frames\": %d, \"arith\": \"%s\", \"messages\": %zu, \"bare_process_us_per_msg\": %.3f, "
                "\"bare_enqueue_us_per_msg\": %.3f, \"graph_drop_us_per_msg\": %.3f, \"graph_over_bare_enqueue_rate\": %.4f, "
                "\"enqueue_over_process_rate\": %.4f, \"queued\": %ld, \"synchronised\": %ld, \"mallocs_in_timed_region\": %llu}\n",
                nch, log2f, mode_name.c_str(), nmsg, bare_process, bare_enqueue, graph_us, bare_enqueue / graph_us, bare_process / bare_enqueue, q, sy, mallocs);
    std::fflush(stdout);
    return 0;
}

static int bench_planes(int log2r, int nchan)
{
    if (log2r < 6 || log2r > 24 || nchan < 1 || nchan > 4096) { std::fprintf(stderr, "bench_planes: 6 <= log2_rows <= 24, 1 <= nchan <= 4096\n"); return 2; }
    const size_t rows = (size_t)1 << log2r, n = rows * (size_t)nchan;
    auto a = dev::make<cf>(n), b = dev::make<cf>(n);
    dev::check(redio_synth_iq(a.data(), 0x5EED0005u, 0, n, nullptr));
    dev::check(redio_stream_sync(nullptr));
    dev::BlockStream st(dev::BlockStream::TRANSFER);
    auto timed = [&](auto call) {
        call(); call();
        dev::check(redio_stream_sync(st));
        double best = 1e30;
        for (int rep = 0; rep < 5; ++rep) {
            const int k = 4;
            auto t0 = clk::now();
            for (int i = 0; i < k; ++i) call();
            dev::check(redio_stream_sync(st));
            best = std::min(best, secs(t0, clk::now()) / k * 1e6);
        }
        return best;
    };
    const double to_planes = timed([&] { dev::check(redio_rows_to_planes_c32(a.data(), rows, nchan, b.data(), rows, st)); });
    const double to_rows = timed([&] { dev::check(redio_planes_to_rows_c32(b.data(), rows, rows, nchan, a.data(), st)); });
    const double copy = timed([&] { dev::check(redio_copy(b.data(), a.data(), n * sizeof(cf), st)); });
    const double gb = 2.0 * (double)n * sizeof(cf) * 1e-3; // read + written, per microsecond = GB/s
    std::printf("{\"mode\": \"bench_planes\", \"log2_rows\": %d, \"nchan\": %d, \"rows_to_planes_us\": %.2f, \"planes_to_rows_us\": %.2f, \"copy_us\": %.2f, "
                "\"rows_to_planes_gbps\": %.1f, \"planes_to_rows_gbps\": %.1f, \"copy_gbps\": %.1f, \"rows_to_planes_over_copy\": %.3f, \"planes_to_rows_over_copy\": %.3f}\n",
                log2r, nchan, to_planes, to_rows, copy, gb / to_planes, gb / to_rows, gb / copy, copy / to_planes, copy / to_rows);
    return 0;
}

int main(int argc, char **argv)
{
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        if (mode == "src_gpu") return src_gpu();
        if (mode == "c4c3") return c4c3();
        if (mode == "bench" && argc == 5) return bench(std::atoi(argv[2]), std::atoi(argv[3]), argv[4]);
        if (mode == "bench_planes" && argc == 4) return bench_planes(std::atoi(argv[2]), std::atoi(argv[3]));
        std::fprintf(stderr, "usage: kpn_src_tests src_gpu | c4c3 | bench nch log2_frames exact|fast | bench_planes log2_rows nchan\n");
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
}
