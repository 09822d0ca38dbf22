// The oversampled synthesis bank's two kernels run on the CPU: a stand-alone program.
//
//   emu_pfb_os_synth wave P fused hops_per_wave hops first_row in.bin taps.bin want.bin
// The fused kernel (libredio_amd/csrc/pfb_os_synth_kernels.hip, pfb_os_synth64_kernel: 64 channels, hop 32): every wavefront of a launch
// (hops_per_wave 0: the launcher's own choice, pfb_os_synth_core.h), sixty-four lanes one at a time through the kernel's own phases --
// the clamped row loads (the request for the next tile included), exchange 1, inverse passes A/B, exchange 2, inverse pass C,
// exchange 3, the skewed reads of the tile with the carried row, the rotating window, the fold and the store predicate.  A phase ends
// where the kernel has a wave_lds_fence(); the tile is poisoned with NaNs before every exchange's stores, so a load of an element that
// exchange did not write shows in the output.  in.bin: (hops + 2 P - 1) * 64 cf32; want.bin: 32 hops cf32 (tests/pfb_os_synth_ref.py).
// Prints the wave count.
//
//   emu_pfb_os_synth ola M P H fused hops first_row chunk w.bin taps.bin want.bin
// The two-pass route's overlap-add pass (pfb_os_synth_ola_kernel) in passes of `chunk` input rows as redio_pfb_os_synth_enqueue cuts
// them (pfb_bank_cut.h): every thread of every launch, its column, its taps and its store.  w.bin: (hops + L - 1) * M cf32, the rows BEHIND the inverse
// transform; want.bin: hops * H cf32.  Prints the pass count.
//
// Every load is fenced inside its buffer (a pass's scratch holds the pass's rows only), every LDS index inside the wave's tile, every
// store inside the output, and every output must be written exactly once.  Exit status 0 only if every check held and the output has
// want.bin's bits.
#include "../../libredio_amd/csrc/pfb_bank_cut.h"
#include "../../libredio_amd/csrc/pfb_os_synth_core.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace redio;

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            std::fprintf(stderr, "emu_pfb_os_synth: %s:%d: %s\n", __FILE__, __LINE__, #c); \
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
    CHECK(std::fgetc(f) == EOF); // exactly n: the fences below are the file's own size
    std::fclose(f);
    return v;
}

struct Out { // the output buffer with fenced stores that count
    std::vector<float2> v;
    std::vector<int> writes;
    explicit Out(size_t n) : v(n), writes(n, 0) {}
    void store(long i, float2 a) { CHECK(i >= 0 && i < (long)v.size()); v[(size_t)i] = a; ++writes[(size_t)i]; }
    void once() const { for (int w : writes) CHECK(w == 1); }
};

template <int P, bool FUSED>
long run_wave(const std::vector<float2> &x, const std::vector<float> &h, const std::vector<float2> &tw, Out &out, long hops, long hpw, int fpar)
{
    constexpr int L = 2 * P;
    const long n_in = (long)x.size();
    if (hpw <= 0) hpw = pfboss_hops_per_wave(hops);
    CHECK(hpw % PFB_TILE == 0); // what the window's in-place rotation and the parity of a tile's rows stand on
    long nwaves = 0;
    auto in_index = [&](long r, int lane) {
        const long i = PFB_M * pfboss_in_row(r, hops, P) + lane;
        CHECK(i >= 0 && i < n_in);
        return i;
    };
    for (long t0 = 0; t0 < hops; t0 += hpw, ++nwaves) {
        CHECK(t0 % 2 == 0);
        const long t1 = t0 + hpw < hops ? t0 + hpw : hops, r_end = t1 + L - 1;
        Tile lds;
        float g[64][L];
        float2 win[64][L], carry[64], v[64][16], rows[64][PFB_TILE];
        float2 twa1[4], twa2[4], twa3[4], twc1[64][4], twc2[64][4], twc3[64][4];
        int early[64], x3[64], opos[64];
        for (int k2 = 0; k2 < 4; ++k2) { twa1[k2] = tw[4 * k2]; twa2[k2] = tw[8 * k2]; twa3[k2] = tw[12 * k2]; }
        for (int lane = 0; lane < 64; ++lane) {
            early[lane] = pfboss_early(lane, fpar);
            x3[lane] = pfboss_x3_base(lane, early[lane]);
            opos[lane] = pfboss_out_pos(lane, early[lane]);
            for (int k = 0; k < L; ++k) {
                const int t = pfboss_tap64(lane, k);
                CHECK(t >= 0 && t < (int)h.size());
                g[lane][k] = h[(size_t)t];
                win[lane][k] = make_float2(0.f, 0.f);
            }
            carry[lane] = make_float2(0.f, 0.f);
            for (int k2 = 0; k2 < 4; ++k2) {
                const int k = k2 + 4 * (lane & 3);
                twc1[lane][k2] = tw[k]; twc2[lane][k2] = tw[2 * k]; twc3[lane][k2] = tw[3 * k];
            }
            for (int ti = 0; ti < PFB_TILE; ++ti) rows[lane][ti] = x[(size_t)in_index(t0 + ti, lane)];
        }
        int par = 0;
        for (long rb = t0; rb < r_end; rb += PFB_TILE, par ^= 1) {
            lds.poison();
            for (int lane = 0; lane < 64; ++lane)
                for (int ti = 0; ti < PFB_TILE; ++ti) lds.at(pfb_x1_store(ti, lane)) = rows[lane][ti];
            for (int lane = 0; lane < 64; ++lane) // the request for the next tile, which the kernel never skips
                for (int ti = 0; ti < PFB_TILE; ++ti) rows[lane][ti] = x[(size_t)in_index(rb + PFB_TILE + ti, lane)];
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
            for (int lane = 0; lane < 64; ++lane) {
                for (int u = 0; u < PFB_TILE / 2; ++u) {
                    const int ti = 2 * u, s = pfboss_slot_new(par, u, P);
                    CHECK(s >= 0 && s + 1 < L);
                    if (u == 0) {
                        const float2 first = lds.at(pfbs_x3_load(0, lane));
                        win[lane][s] = early[lane] ? carry[lane] : first;
                    } else {
                        win[lane][s] = lds.at(pfboss_x3_load(x3[lane], ti));
                    }
                    win[lane][s + 1] = lds.at(pfboss_x3_load(x3[lane], ti + 1));
                    float2 acc = make_float2(0.f, 0.f);
                    for (int k = 0; k < L; ++k) {
                        const int sl = pfboss_slot(par, u, k, P);
                        CHECK(sl >= 0 && sl < L);
                        acc = mac<FUSED>(win[lane][sl], g[lane][k], acc);
                    }
                    const long q0 = pfboss_hop(rb + ti, P);
                    const bool st_early = q0 >= t0 && q0 < t1, st_late = q0 + 1 >= t0 && q0 + 1 < t1;
                    if (early[lane] ? st_early : st_late) {
                        CHECK(opos[lane] >= 0 && opos[lane] < 64);
                        out.store(PFBOS_H * q0 + opos[lane], acc);
                    }
                }
                carry[lane] = lds.at(pfbs_x3_load(PFB_TILE - 1, lane));
            }
        }
    }
    return nwaves;
}

template <bool FUSED>
long run_ola(const std::vector<float2> &w, const std::vector<float> &h, Out &out, long hops, long M, long P, long H, unsigned long long F, long chunk)
{
    const long L = pfboss_L(M, P, H);
    const long T = hops + L - 1;
    CHECK((long)w.size() == T * M);
    const BankCut cut = bank_cut_os_synth((size_t)M, (size_t)P, (size_t)H);
    CHECK(cut.min_rows == (size_t)L);
    const size_t chunk_rows = bank_chunk_rows(cut, (size_t)chunk); // fewer than L rows count as L
    const long passes = (long)bank_passes(cut, chunk_rows, (size_t)hops);
    for (long i = 0; i < passes; ++i) {
        const BankPass ps = bank_pass(cut, chunk_rows, (size_t)hops, (size_t)i);
        const long c0 = (long)ps.first, n = (long)ps.units;
        CHECK(ps.rows <= bank_pass_rows(cut, chunk_rows, (size_t)hops)); // inside the scratch that reserve sized
        const long f0 = (long)((F + (unsigned long long)c0) % (unsigned long long)M);
        const long wo = (long)ps.in_off, wn = (long)ps.rows * M; // the pass's scratch: rows c0 .. c0 + n + L - 2 behind the transform
        CHECK(wo + wn <= (long)w.size());
        const long nout = n * H, nthreads = ((nout + 255) / 256) * 256;
        for (long e = 0; e < nthreads; ++e) {
            if (e >= nout) continue;
            const long q = e / H, j = e - q * H;
            const long c = pfboss_col(f0, q, j, M, H, L);
            CHECK(c >= 0 && c < M);
            // tau mod M in 128-bit arithmetic on the whole call's indices
            CHECK((unsigned long long)c == (unsigned long long)((((unsigned __int128)F + (unsigned __int128)(L - 1 + c0 + q)) * (unsigned __int128)H + (unsigned __int128)j) % (unsigned __int128)M));
            float2 acc = make_float2(0.f, 0.f);
            for (long k = pfboss_k0(j, M, P, H, L); k < L; ++k) {
                const long o = pfboss_offset(k, j, H, L), t = pfboss_tap(o, M, P);
                CHECK(o >= 0 && o < P * M && t >= 0 && t < (long)h.size());
                const long i = (q + k) * M + c;
                CHECK(i >= 0 && i < wn);
                acc = mac<FUSED>(w[(size_t)(wo + i)], h[(size_t)t], acc);
            }
            if (pfboss_k0(j, M, P, H, L)) CHECK(pfboss_offset(0, j, H, L) >= P * M); // the row left out is outside its window
            out.store((long)ps.out_off + e, acc);
        }
    }
    return passes;
}

int same_bits(const std::vector<float2> &a, const std::vector<float2> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float2)) == 0);
}
} // namespace

int main(int argc, char **argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "wave" && argc == 10) {
        const int P = std::atoi(argv[2]), fused = std::atoi(argv[3]);
        const long hpw = std::atol(argv[4]), hops = std::atol(argv[5]);
        const unsigned long long F = std::strtoull(argv[6], nullptr, 10);
        CHECK(hops >= 1 && (P == 4 || P == 8 || P == 16));
        const std::vector<float2> x = read_all<float2>(argv[7], (size_t)(hops + 2 * P - 1) * PFB_M);
        const std::vector<float> h = read_all<float>(argv[8], (size_t)PFB_M * P);
        const std::vector<float2> want = read_all<float2>(argv[9], (size_t)hops * PFBOS_H);
        Out out((size_t)hops * PFBOS_H);
        // the inverse plan's table: evaluated in double and rounded once, phase = + 2 pi i / 64 (kiss_fft_alloc with inverse_fft)
        std::vector<float2> tw(PFB_M);
        const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
        for (int i = 0; i < PFB_M; ++i) {
            double phase = -2 * pi * i / PFB_M;
            phase *= -1;
            tw[(size_t)i] = make_float2((float)std::cos(phase), (float)std::sin(phase));
        }
        long nwaves = 0;
        const int fpar = (int)(F & 1);
        switch (P * 2 + (fused ? 1 : 0)) {
        case 8: nwaves = run_wave<4, false>(x, h, tw, out, hops, hpw, fpar); break;
        case 9: nwaves = run_wave<4, true>(x, h, tw, out, hops, hpw, fpar); break;
        case 16: nwaves = run_wave<8, false>(x, h, tw, out, hops, hpw, fpar); break;
        case 17: nwaves = run_wave<8, true>(x, h, tw, out, hops, hpw, fpar); break;
        case 32: nwaves = run_wave<16, false>(x, h, tw, out, hops, hpw, fpar); break;
        default: nwaves = run_wave<16, true>(x, h, tw, out, hops, hpw, fpar); break;
        }
        out.once();
        CHECK(same_bits(out.v, want));
        std::printf("%ld\n", nwaves);
        return 0;
    }
    if (mode == "ola" && argc == 12) {
        const long M = std::atol(argv[2]), P = std::atol(argv[3]), H = std::atol(argv[4]);
        const int fused = std::atoi(argv[5]);
        const long hops = std::atol(argv[6]);
        const unsigned long long F = std::strtoull(argv[7], nullptr, 10);
        const long chunk = std::atol(argv[8]);
        CHECK(M >= 1 && P >= 1 && H >= 1 && H <= M && hops >= 1 && chunk >= 1);
        const long L = pfboss_L(M, P, H);
        const std::vector<float2> w = read_all<float2>(argv[9], (size_t)((hops + L - 1) * M));
        const std::vector<float> h = read_all<float>(argv[10], (size_t)(M * P));
        const std::vector<float2> want = read_all<float2>(argv[11], (size_t)(hops * H));
        Out out((size_t)(hops * H));
        const long passes = fused ? run_ola<true>(w, h, out, hops, M, P, H, F, chunk) : run_ola<false>(w, h, out, hops, M, P, H, F, chunk);
        out.once();
        CHECK(same_bits(out.v, want));
        std::printf("%ld\n", passes);
        return 0;
    }
    std::fprintf(stderr, "usage: emu_pfb_os_synth wave P fused hops_per_wave hops first_row in.bin taps.bin want.bin\n"
                         "       emu_pfb_os_synth ola M P H fused hops first_row chunk w.bin taps.bin want.bin\n");
    return 1;
}
