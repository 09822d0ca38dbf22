// The oversampled channelizer's two kernels run on the CPU: a stand-alone program.
//
//   emu_pfb_os wave P fused rows first_row in.bin taps.bin want.bin
// The fused kernel (libredio_amd/csrc/pfb_os_kernels.hip, pfb_os64_kernel: 64 channels, hop 32): every wavefront of a launch under the
// launcher's geometry (pfb_os_core.h), sixty-four lanes one at a time through the kernel's own phases -- the window prologue, the clamped
// half-row loads (the prefetch of the next tile included), the two interleaved windows, the fold, exchange 1 with the shift in its lane
// index, passes A/B, exchange 2, pass C and both forms of the store.  A phase ends where the kernel has a wave_lds_fence(); the tile is
// poisoned with NaNs before every exchange's stores, so a load of an element that exchange did not write shows in the output.
// in.bin: 32 (rows - 1) + 64 P cf32; want.bin: rows * 64 cf32 (the rows of tests/pfb_os_ref.py).  Prints the wave count.
//
//   emu_pfb_os branch M P H fused rows first_row chunk in.bin taps.bin want.bin
// The two-pass route's branch pass (pfb_os_kernels.hip, pfb_os_branch_kernel) in passes of `chunk` rows as redio_pfb_os_enqueue cuts them (pfb_bank_cut.h):
// every thread of every launch, its loads, the shift and the rotated store.  in.bin: H (rows - 1) + M P cf32; want.bin: rows * M cf32,
// the rotated branch sums in front of the transform.  Prints the pass count.
//
// Every stream load is fenced inside [0, n_in), every LDS index inside the wave's tile, every store inside rows * M, and every output
// must be written exactly once.  Exit status 0 only if every check held and the output has want.bin's bits.
#include "../../libredio_amd/csrc/pfb_bank_cut.h"
#include "../../libredio_amd/csrc/pfb_os_core.h"
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
            std::fprintf(stderr, "emu_pfb_os: %s:%d: %s\n", __FILE__, __LINE__, #c); \
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
long run_wave(const std::vector<float2> &x, const std::vector<float> &h, const std::vector<float2> &tw, Out &out, Out &narrow, long rows, int fpar)
{
    const long n_in = (long)x.size();
    const long rpw = pfbos_rows_per_wave(rows);
    CHECK(rpw % PFB_TILE == 0 && rpw >= 4 * PFB_TILE);
    long nwaves = 0;
    auto ld = [&](long q, int lane) { // one lane of a half-row request, clamped as the kernel clamps it
        const long i = pfbos_in_index(pfbos_half(q, rows, P), lane);
        CHECK(i >= 0 && i < n_in);
        return x[(size_t)i];
    };
    for (long t0 = 0; t0 < rows; t0 += rpw, ++nwaves) {
        CHECK(t0 % 2 == 0); // what the parity of F + ti stands on
        const long t1 = t0 + rpw < rows ? t0 + rpw : rows;
        Tile lds;
        float g[64][P];
        float2 win[64][2][P], v[64][16];
        float2 twa1[4], twa2[4], twa3[4], twc1[64][4], twc2[64][4], twc3[64][4];
        for (int k2 = 0; k2 < 4; ++k2) { twa1[k2] = tw[4 * k2]; twa2[k2] = tw[8 * k2]; twa3[k2] = tw[12 * k2]; }
        for (int lane = 0; lane < 64; ++lane) {
            for (int p = 0; p < P; ++p) g[lane][p] = h[(size_t)(PFB_M * p + lane)];
            for (int k2 = 0; k2 < 4; ++k2) {
                const int k = k2 + 4 * (lane & 3);
                twc1[lane][k2] = tw[k]; twc2[lane][k2] = tw[2 * k]; twc3[lane][k2] = tw[3 * k];
            }
            const float q = std::numeric_limits<float>::quiet_NaN();
            for (int par = 0; par < 2; ++par) {
                for (int p = 0; p < P; ++p) win[lane][par][p] = make_float2(q, q);
                for (int p = 0; p < P - 1; ++p) { // the prologue is NOT clamped in the kernel: it must be inside the stream as it stands
                    const long i = pfbos_in_index(t0 + par + 2 * p, lane);
                    CHECK(i >= 0 && i < n_in);
                    win[lane][par][pfbos_slot(0, p, P)] = x[(size_t)i];
                }
            }
        }
        int tile_no = 0;
        for (long tb = t0; tb < t1; tb += PFB_TILE, ++tile_no) {
            const int J0 = (tile_no & 1) ? PFB_TILE / 2 : 0; // the kernel's pair of tiles
            for (int lane = 0; lane < 64; ++lane) // the request for the next tile, which the kernel never skips: addresses only
                for (int ti = 0; ti < PFB_TILE; ++ti) ld(pfbos_enter(tb + PFB_TILE, P) + ti, lane);
            lds.poison();
            for (int lane = 0; lane < 64; ++lane)
                for (int ti = 0; ti < PFB_TILE; ++ti) {
                    const int par = ti & 1, j = J0 + (ti >> 1);
                    win[lane][par][pfbos_slot(j, P - 1, P)] = ld(pfbos_enter(tb, P) + ti, lane);
                    float2 acc = make_float2(0.f, 0.f);
                    for (int p = 0; p < P; ++p) acc = mac<FUSED>(win[lane][par][pfbos_slot(j, p, P)], g[lane][p], acc);
                    lds.at(pfb_x1_store(ti, pfbos_x1_lane(lane, ti, fpar))) = acc;
                }
            for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 16; ++e) v[lane][e] = lds.at(pfb_x1_load(lane, e));
            lds.poison();
            for (int lane = 0; lane < 64; ++lane) {
                pfb_fft64_passAB_pre<false>(v[lane], tw[0], twa1, twa2, twa3);
                for (int k2 = 0; k2 < 4; ++k2)
                    for (int k1 = 0; k1 < 4; ++k1) lds.at(pfb_x2_store(lane, k1, k2)) = v[lane][k1 + 4 * k2];
            }
            for (int lane = 0; lane < 64; ++lane)
                for (int f = 0; f < 16; ++f) v[lane][f] = lds.at(pfb_x2_load(lane, f));
            for (int lane = 0; lane < 64; ++lane) {
                pfb_fft64_passC_pre<false>(v[lane], twc1[lane], twc2[lane], twc3[lane]);
                const long row = tb + (lane >> 2);
                if (row >= t1) continue;
                const long o = PFB_M * tb + PFB_M * (lane >> 2) + 4 * (lane & 3); // orow
                for (int k0 = 0; k0 < 4; ++k0) {
                    // the wide form: two 16-byte stores, (v[k0], v[k0 + 4]) and (v[k0 + 8], v[k0 + 12])
                    out.store(o + 16 * k0, v[lane][k0]); out.store(o + 16 * k0 + 1, v[lane][k0 + 4]);
                    out.store(o + 16 * k0 + 2, v[lane][k0 + 8]); out.store(o + 16 * k0 + 3, v[lane][k0 + 12]);
                    // the 8-byte form
                    for (int k2 = 0; k2 < 4; ++k2) narrow.store(o + 16 * k0 + k2, v[lane][k0 + 4 * k2]);
                    for (int k2 = 0; k2 < 4; ++k2) CHECK(o + 16 * k0 + k2 == PFB_M * row + pfb_out_channel(lane, k0, k2));
                }
            }
        }
    }
    CHECK(nwaves == pfbos_waves(rows));
    return nwaves;
}

// pfb_os_branch_kernel, every thread of every pass
template <bool FUSED>
long run_branch(const std::vector<float2> &x, const std::vector<float> &h, Out &out, long rows, int M, int P, long H, unsigned long long F, long chunk)
{
    const long n_in = (long)x.size();
    const BankCut cut = bank_cut_os((size_t)M, (size_t)P, (size_t)H);
    const size_t chunk_rows = bank_chunk_rows(cut, (size_t)chunk);
    const long passes = (long)bank_passes(cut, chunk_rows, (size_t)rows);
    for (long i = 0; i < passes; ++i) {
        const BankPass ps = bank_pass(cut, chunk_rows, (size_t)rows, (size_t)i);
        const long c0 = (long)ps.first, n = (long)ps.units;
        CHECK(ps.rows <= bank_pass_rows(cut, chunk_rows, (size_t)rows)); // inside the scratch that reserve sized
        const long f0 = (long)((F + (unsigned long long)c0) % (unsigned long long)M);
        const long xo = (long)ps.in_off, vo = (long)ps.out_off; // the pass's pointers: d_in + c0 H; the scratch rows land at out + c0 M behind the transform
        const long nthreads = ((n * M + 255) / 256) * 256;
        for (long e = 0; e < nthreads; ++e) {
            if (e >= n * M) continue;
            const long r = e / M;
            const int m = (int)(e - r * M);
            float2 acc = make_float2(0.f, 0.f);
            for (int p = 0; p < P; ++p) {
                const long i = xo + r * H + m + (long)p * M;
                CHECK(i >= 0 && i < n_in);
                CHECK((long)p * M + m < (long)h.size());
                acc = mac<FUSED>(x[(size_t)i], h[(size_t)((long)p * M + m)], acc);
            }
            const long s = pfbos_shift(f0, r, M, H), k = pfbos_rot(m, s, M);
            CHECK(s >= 0 && s < M && k >= 0 && k < M);
            CHECK((unsigned long long)s == ((F + (unsigned long long)(c0 + r)) % (unsigned long long)M) * (unsigned long long)H % (unsigned long long)M);
            CHECK(r * M + k < (long)ps.rows * M); // inside the pass's scratch
            out.store(vo + r * M + k, acc);
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
    if (mode == "wave" && argc == 9) {
        const int P = std::atoi(argv[2]), fused = std::atoi(argv[3]);
        const long rows = std::atol(argv[4]);
        const unsigned long long F = std::strtoull(argv[5], nullptr, 10);
        CHECK(rows >= 1 && (P == 4 || P == 8 || P == 16));
        const std::vector<float2> x = read_all<float2>(argv[6], (size_t)(PFBOS_H * (rows - 1) + PFB_M * P));
        const std::vector<float> h = read_all<float>(argv[7], (size_t)PFB_M * P);
        const std::vector<float2> want = read_all<float2>(argv[8], (size_t)rows * PFB_M);
        Out out((size_t)rows * PFB_M), narrow((size_t)rows * PFB_M);
        // the forward plan's table: evaluated in double and rounded once, phase = - 2 pi i / 64 (kiss_fft_alloc)
        std::vector<float2> tw(PFB_M);
        const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
        for (int i = 0; i < PFB_M; ++i) {
            const double phase = -2 * pi * i / PFB_M;
            tw[(size_t)i] = make_float2((float)std::cos(phase), (float)std::sin(phase));
        }
        long nwaves = 0;
        const int fpar = (int)(F & 1);
        switch (P * 2 + (fused ? 1 : 0)) {
        case 8: nwaves = run_wave<4, false>(x, h, tw, out, narrow, rows, fpar); break;
        case 9: nwaves = run_wave<4, true>(x, h, tw, out, narrow, rows, fpar); break;
        case 16: nwaves = run_wave<8, false>(x, h, tw, out, narrow, rows, fpar); break;
        case 17: nwaves = run_wave<8, true>(x, h, tw, out, narrow, rows, fpar); break;
        case 32: nwaves = run_wave<16, false>(x, h, tw, out, narrow, rows, fpar); break;
        default: nwaves = run_wave<16, true>(x, h, tw, out, narrow, rows, fpar); break;
        }
        out.once();
        narrow.once();
        CHECK(same_bits(out.v, want) && same_bits(narrow.v, want));
        std::printf("%ld\n", nwaves);
        return 0;
    }
    if (mode == "branch" && argc == 12) {
        const int M = std::atoi(argv[2]), P = std::atoi(argv[3]);
        const long H = std::atol(argv[4]);
        const int fused = std::atoi(argv[5]);
        const long rows = std::atol(argv[6]);
        const unsigned long long F = std::strtoull(argv[7], nullptr, 10);
        const long chunk = std::atol(argv[8]);
        CHECK(M >= 1 && P >= 1 && H >= 1 && H <= M && rows >= 1 && chunk >= 1);
        const std::vector<float2> x = read_all<float2>(argv[9], (size_t)(H * (rows - 1) + (long)M * P));
        const std::vector<float> h = read_all<float>(argv[10], (size_t)M * P);
        const std::vector<float2> want = read_all<float2>(argv[11], (size_t)rows * M);
        Out out((size_t)rows * M);
        const long passes = fused ? run_branch<true>(x, h, out, rows, M, P, H, F, chunk) : run_branch<false>(x, h, out, rows, M, P, H, F, chunk);
        out.once();
        CHECK(same_bits(out.v, want));
        std::printf("%ld\n", passes);
        return 0;
    }
    std::fprintf(stderr, "usage: emu_pfb_os wave P fused rows first_row in.bin taps.bin want.bin\n"
                         "       emu_pfb_os branch M P H fused rows first_row chunk in.bin taps.bin want.bin\n");
    return 1;
}
