// The fused synthesis filterbank (libredio_amd/csrc/pfb_synth_kernels.hip, pfb_synth64_kernel) run on the CPU: a stand-alone program
// that takes every wavefront of a launch through the kernel's own phases, sixty-four lanes one at a time -- the clamped row loads (the
// prefetch of the next tile included), exchange 1, inverse passes A/B, exchange 2, inverse pass C, exchange 3, the rotating window, the
// fold and the store predicate (pfb_synth_core.h, pfb_core.h).  A phase ends where the kernel has a wave_lds_fence(); the tile is
// poisoned with NaNs before every exchange's stores, so a load of an element that exchange did not write shows in the output.  Every
// LDS index is checked against the wave's PFB_LDS tile and every global index against its buffer; every output is written exactly once.
//
//   emu_pfb_synth P fused rows_per_wave rows in.bin taps.bin out.bin
// in.bin: (rows + P - 1) * 64 cf32; taps.bin: 64 P f32; out.bin: rows * 64 cf32; rows_per_wave 0: the launcher's own choice.
// Prints the wave count.  Exit status 0 only if every check held.
#include "../../libredio_amd/csrc/pfb_synth_core.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

using namespace redio;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "emu_pfb_synth: %s:%d: %s\n", __FILE__, __LINE__, #c); \
            std::exit(2);                                                     \
        }                                                                     \
    } while (0)

namespace {
struct Tile { // the wave's LDS tile with range-checked indices
    std::vector<float2> m = std::vector<float2>(PFB_LDS);
    float2 &at(int i) { CHECK(i >= 0 && i < PFB_LDS); return m[(size_t)i]; }
    void poison() { const float q = std::numeric_limits<float>::quiet_NaN(); for (auto &e : m) e = make_float2(q, q); }
};

template <typename T>
std::vector<T> read_all(const char *path, size_t n)
{
    std::vector<T> v(n);
    FILE *f = std::fopen(path, "rb");
    CHECK(f != nullptr);
    CHECK(std::fread(v.data(), sizeof(T), n, f) == n);
    std::fclose(f);
    return v;
}

template <int P, bool FUSED>
long run(const std::vector<float2> &x, const std::vector<float> &h, const std::vector<float2> &tw, std::vector<float2> &out, long rows, long rpw)
{
    const long n_in = (long)x.size(), n_out = (long)out.size();
    std::vector<int> writes((size_t)n_out, 0);
    if (rpw <= 0) rpw = pfbs_rows_per_wave(rows);
    CHECK(rpw % PFB_TILE == 0); // what the window's in-place rotation needs of a run's first tile
    long nwaves = 0;
    auto in_index = [&](long r, int lane) {
        const long i = PFB_M * pfbs_in_row(r, rows, P) + lane;
        CHECK(i >= 0 && i < n_in);
        return i;
    };
    for (long t0 = 0; t0 < rows; t0 += rpw, ++nwaves) {
        const long t1 = t0 + rpw < rows ? t0 + rpw : rows, r_end = t1 + P - 1;
        Tile lds;
        float g[64][P];
        float2 win[64][P], v[64][16];
        float2 twa1[4], twa2[4], twa3[4], twc1[64][4], twc2[64][4], twc3[64][4];
        for (int k2 = 0; k2 < 4; ++k2) { twa1[k2] = tw[4 * k2]; twa2[k2] = tw[8 * k2]; twa3[k2] = tw[12 * k2]; }
        for (int lane = 0; lane < 64; ++lane) {
            for (int p = 0; p < P; ++p) { g[lane][p] = h[(size_t)(PFB_M * p + lane)]; win[lane][p] = make_float2(0.f, 0.f); }
            for (int k2 = 0; k2 < 4; ++k2) {
                const int k = k2 + 4 * (lane & 3);
                twc1[lane][k2] = tw[k]; twc2[lane][k2] = tw[2 * k]; twc3[lane][k2] = tw[3 * k];
            }
        }
        for (long rb = t0; rb < r_end; rb += PFB_TILE) {
            for (int lane = 0; lane < 64; ++lane) // the request for the next tile, which the kernel never skips: addresses only
                for (int ti = 0; ti < PFB_TILE; ++ti) in_index(rb + PFB_TILE + ti, lane);
            lds.poison();
            for (int lane = 0; lane < 64; ++lane)
                for (int ti = 0; ti < PFB_TILE; ++ti) lds.at(pfb_x1_store(ti, lane)) = x[(size_t)in_index(rb + ti, lane)];
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 16; ++e) v[lane][e] = lds.at(pfb_x1_load(lane, e));
            lds.poison();
            for (int lane = 0; lane < 64; ++lane) {
                pfb_fft64_passAB_pre<true>(v[lane], tw[0], twa1, twa2, twa3);
                for (int k2 = 0; k2 < 4; ++k2)
                    for (int k1 = 0; k1 < 4; ++k1) lds.at(pfb_x2_store(lane, k1, k2)) = v[lane][k1 + 4 * k2];
            }
            for (int lane = 0; lane < 64; ++lane)
                for (int f = 0; f < 16; ++f) v[lane][f] = lds.at(pfb_x2_load(lane, f));
            lds.poison();
            for (int lane = 0; lane < 64; ++lane) {
                pfb_fft64_passC_pre<true>(v[lane], twc1[lane], twc2[lane], twc3[lane]);
                for (int k0 = 0; k0 < 4; ++k0)
                    for (int k2 = 0; k2 < 4; ++k2) lds.at(pfbs_x3_store(lane, k0, k2)) = v[lane][k0 + 4 * k2];
            }
            for (int lane = 0; lane < 64; ++lane)
                for (int ti = 0; ti < PFB_TILE; ++ti) {
                    win[lane][(ti + P - 1) % P] = lds.at(pfbs_x3_load(ti, lane));
                    float2 acc = make_float2(0.f, 0.f);
                    for (int p = 0; p < P; ++p) acc = mac<FUSED>(win[lane][(ti + p) % P], g[lane][p], acc);
                    if (pfbs_stores(rb + ti, t0, t1, P)) {
                        const long o = PFB_M * (rb + ti - (P - 1)) + lane;
                        CHECK(o >= 0 && o < n_out);
                        out[(size_t)o] = acc;
                        ++writes[(size_t)o];
                    }
                }
        }
    }
    for (long i = 0; i < n_out; ++i) CHECK(writes[(size_t)i] == 1);
    return nwaves;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc != 8) { std::fprintf(stderr, "usage: emu_pfb_synth P fused rows_per_wave rows in.bin taps.bin out.bin\n"); return 1; }
    const int P = std::atoi(argv[1]), fused = std::atoi(argv[2]);
    const long rpw = std::atol(argv[3]), rows = std::atol(argv[4]);
    CHECK(rows >= 1 && (P == 4 || P == 8 || P == 16));
    const std::vector<float2> x = read_all<float2>(argv[5], (size_t)(rows + P - 1) * PFB_M);
    const std::vector<float> h = read_all<float>(argv[6], (size_t)PFB_M * P);
    std::vector<float2> out((size_t)rows * PFB_M);
    // the inverse plan's table: evaluated in double and rounded once, phase = + 2 pi i / 64 (kiss_fft_alloc with inverse_fft)
    std::vector<float2> tw(PFB_M);
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
    for (int i = 0; i < PFB_M; ++i) {
        double phase = -2 * pi * i / PFB_M;
        phase *= -1;
        tw[(size_t)i] = make_float2((float)std::cos(phase), (float)std::sin(phase));
    }
    long nwaves = 0;
    switch (P * 2 + (fused ? 1 : 0)) {
    case 8: nwaves = run<4, false>(x, h, tw, out, rows, rpw); break;
    case 9: nwaves = run<4, true>(x, h, tw, out, rows, rpw); break;
    case 16: nwaves = run<8, false>(x, h, tw, out, rows, rpw); break;
    case 17: nwaves = run<8, true>(x, h, tw, out, rows, rpw); break;
    case 32: nwaves = run<16, false>(x, h, tw, out, rows, rpw); break;
    default: nwaves = run<16, true>(x, h, tw, out, rows, rpw); break;
    }
    FILE *f = std::fopen(argv[7], "wb");
    CHECK(f != nullptr);
    CHECK(std::fwrite(out.data(), sizeof(float2), out.size(), f) == out.size());
    std::fclose(f);
    std::printf("%ld\n", nwaves);
    return 0;
}
