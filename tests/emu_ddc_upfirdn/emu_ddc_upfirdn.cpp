// emu_ddc_upfirdn.cpp -- CPU emulation of the tuned resampler's kernels (libredio_amd/csrc/ddc_upfirdn_kernels.hip): every thread of every
// workgroup of a call runs route 1 -- the tuner's loader policy (ddc_core.h, DdcTile<U8>::load) into the resampler's image, then the
// resampler's phase loop and store loop (upfirdn_core.h) -- the very sources the device compiles, against fenced copies of the stream
// (cf32 and bytes), the oscillator table, the polyphase taps, the LDS allocation and the output; the direct kernel's per-thread function
// (ddc_upfirdn_core.h) runs on the same calls.  Outputs are compared bit for bit with the contract written out (include/redio.h: the
// mix, every operation rounded on its own, then the fold over j with the stuffed zeros skipped), and every fence must be intact.
//   the table    exactly L + DDC_TABLE_EXT entries between fences of NaN: a lane that reads outside computes NaN
//   the LDS      the image and the output tile have exactly upfirdn_img_elems and 256 R U' elements, each between fences of NaN 8192
//                elements wide: a lane that reads past the image computes NaN, one that writes past either is found afterwards
//   cf32 stream  exactly n_in samples between fences of NaN
//   byte stream  a heap block that ends with the stream's last byte (a byte cannot hold a NaN: a read past the end is found by the
//                SAN=1 build)
// A stand-alone program: exit status 0 and "emu_ddc_upfirdn ok" when everything held.
//   emu_ddc_upfirdn          twelve shapes, four output counts around the tile each, both folds, cf32 and bytes; oscillator periods
//                            1, 2, 3, 24, 65536 (an odd period gives odd bases: the two-8-byte table path) times five first indices up to
//                            2^64 - 1 - n; the stream aligned, one sample off and at byte offsets 0 to 3; the output aligned and one off
//   emu_ddc_upfirdn --long   long filters: tiles of 52 to 150 KiB (the longest table reads), one whole and one partial tile each
#include "../../libredio_amd/csrc/ddc_upfirdn_core.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

using namespace redio;

namespace {
constexpr int FENCE = 64;       // elements in front of and behind every buffer
constexpr int LDS_FENCE = 8192; // and around the two parts of the LDS allocation: wider than any window's stride past the image
int failures = 0;
long calls = 0;

float value(unsigned &state)
{
    state = state * 1664525u + 1013904223u;
    return (float)(int)(state >> 8) * (1.0f / 8388608.0f) - 1.0f;
}
float nan_of(float) { return NAN; }
float2 nan_of(float2) { return make_float2(NAN, NAN); }
bool same(const float2 &a, const float2 &b) { return std::memcmp(&a, &b, 8) == 0; }

// a buffer between two fences of NaN: a read past an end poisons what is computed from it, a write past an end is found afterwards
template <typename V>
struct Fenced {
    std::vector<V> all; size_t n, fence;
    explicit Fenced(size_t n_, size_t fence_ = FENCE) : all(n_ + 2 * fence_, nan_of(V{})), n(n_), fence(fence_) {}
    V *data() { return all.data() + fence; }
    bool intact() const
    {
        for (size_t i = 0; i < fence; ++i)
            if (!std::isnan(*(const float *)&all[i]) || !std::isnan(*(const float *)&all[fence + n + i])) return false;
        return true;
    }
};

// the oscillator table as the plan lays it out (ddc_upfirdn_api.hip): entry e = w[e mod L], L + DDC_TABLE_EXT entries
struct Table {
    unsigned L; std::vector<float2> w; Fenced<float2> dev;
    explicit Table(unsigned L_) : L(L_), w(L_), dev((size_t)L_ + DDC_TABLE_EXT)
    {
        unsigned st = 0xC0FFEEu + L_;
        for (auto &v : w) { v.x = value(st); v.y = value(st); }
        for (size_t e = 0; e < dev.n; ++e) dev.data()[e] = w[e % L];
    }
};

// ---- the contract, written out ---------------------------------------------------------------------------------------------------------
float2 mix(float2 x, float2 w) // kpn::mul_vecs: four products and two sums, each rounded on its own (built with -ffp-contract=off)
{
    const float a = x.x * w.x, b = x.y * w.y, c = x.x * w.y, d = x.y * w.x;
    return make_float2(a - b, c + d);
}
// m[n] = mix(x[n], w[(first + n) mod L]) for the whole call; bytes go through i2f first (redio_data_to_samples)
std::vector<float2> mixed(const float2 *xc, const unsigned char *xb, long n_in, const Table &t, unsigned long long first)
{
    std::vector<float2> m((size_t)n_in);
    for (long n = 0; n < n_in; ++n) {
        const unsigned e = (unsigned)((first % t.L + (unsigned long long)n % t.L) % t.L); // (first + n) mod L without overflow
        const float2 x = xb ? make_float2(i2f(xb[2 * n]), i2f(xb[2 * n + 1])) : xc[n];
        m[(size_t)n] = mix(x, t.w[e]);
    }
    return m;
}
template <bool FUSED>
float2 contract(const float2 *m, const float *h, long K, long U, long D, long i)
{
    float2 acc{};
    for (long j = 0; j < K; ++j)
        if ((i * D + j) % U == 0) acc = mac<FUSED>(m[(i * D + j) / U], h[j], acc);
    return acc;
}
// the same fold without the K - K / U skipped positions: the first j that meets a sample, then every U-th
template <bool FUSED>
float2 contract_strided(const float2 *m, const float *h, long K, long U, long D, long i)
{
    float2 acc{};
    for (long j = (U - (i * D) % U) % U; j < K; j += U) acc = mac<FUSED>(m[(i * D + j) / U], h[j], acc);
    return acc;
}

// ---- route 1, every thread of every workgroup ----------------------------------------------------------------------------------------
template <bool U8, int DP, int R, bool FUSED>
void tiled_call(const DdcTile<U8> &in, const UpfirdnPhase *ph, const float *taps, int Up, int Wp, float2 *y, long n_out, bool vec_out, int *bad)
{
    constexpr int NT = 256, NQ = NT * R, LSTR = R * DP;
    constexpr bool STREAM = DP >= 2;
    const long img = upfirdn_img_elems(R, DP, Wp), lds = upfirdn_lds_elems(R, Up, DP, Wp);
    const long per_tile = (long)NQ * Up;
    if (lds - img != per_tile || lds * 8 > UPFIRDN_LDS_MAX) ++*bad; // the launch's allocation is the image and the output tile, and fits
    if (!ddc_upfirdn_tile_ok(R, DP, Wp)) ++*bad;                     // the launcher's condition on the table index
    for (long t = 0; t < (n_out + per_tile - 1) / per_tile; ++t) {
        Fenced<float2> image((size_t)img, LDS_FENCE), tile((size_t)(lds - img), LDS_FENCE);
        float2 *xs = image.data(), *ys = tile.data();
        const long in0 = t * NQ * DP;
        for (int tid = 0; tid < NT; ++tid)
            in.template load<STREAM, 4>(tid, in0, (int)upfirdn_tile_in(R, DP, Wp), [&](int n, float2 v) {
                const long at = tile_image_index(n, LSTR);
                if (at < 0 || at >= img) ++*bad; else xs[at] = v;
            });
        for (int tid = 0; tid < NT; ++tid) upfirdn_phases_thread<float2, DP, R, FUSED, 16>(xs, ys, tid, ph, taps, Up);
        for (int tid = 0; tid < NT; ++tid) upfirdn_store_thread<float2, STREAM>(tid, NT, ys, NQ * Up, y + t * per_tile, n_out - t * per_tile, vec_out);
        if (!image.intact() || !tile.intact()) ++*bad;
    }
}

template <bool U8, int DP, bool FUSED>
void tiled_r(int R, const DdcTile<U8> &in, const UpfirdnPhase *ph, const float *taps, int Up, int Wp, float2 *y, long n_out, bool vo, int *bad)
{
    if (R == 4) {
        if constexpr (upfirdn_r_max(DP) >= 4) tiled_call<U8, DP, 4, FUSED>(in, ph, taps, Up, Wp, y, n_out, vo, bad);
        else ++*bad;
    } else if (R == 2) tiled_call<U8, DP, 2, FUSED>(in, ph, taps, Up, Wp, y, n_out, vo, bad);
    else tiled_call<U8, DP, 1, FUSED>(in, ph, taps, Up, Wp, y, n_out, vo, bad);
}

// One call.  xoff: cf32 -- samples off a 16-byte boundary (0, 1); bytes -- the byte offset (0 ... 3).  yoff: samples off a 16-byte
// boundary.  written: the contract's K-step form (every j tested) instead of the strided one
template <bool U8, bool FUSED>
void one_call(long K, long U, long D, long n_in, Table &tab, unsigned long long first, int xoff, int yoff, unsigned seed, bool written)
{
    ++calls;
    const long Up = upfirdn_period_out(U, D), Dp = upfirdn_period_in(U, D), Wp = upfirdn_window(K, U, D);
    const long n_out = (long)upfirdn_nout(n_in, K, U, D);
    unsigned st = seed;
    std::vector<float> h((size_t)K);
    for (float &v : h) v = value(st);
    std::vector<UpfirdnPhase> ph;
    std::vector<float> tp;
    upfirdn_build(h.data(), K, U, D, ph, tp);
    Fenced<float> tbuf(tp.size());
    std::memcpy(tbuf.data(), tp.data(), tp.size() * sizeof(float));
    // the stream: cf32 between NaN fences (the one slack sample is NaN too), on a 16-byte boundary or one sample off it; bytes in a heap
    // block of their own that begins xoff bytes in front of them and ends with the last of them
    Fenced<float2> xbuf(U8 ? 0 : (size_t)n_in + 1);
    std::unique_ptr<unsigned char[]> bbuf(U8 ? new unsigned char[(size_t)(xoff + 2 * n_in)] : nullptr);
    const void *x;
    const float2 *xc = nullptr;
    const unsigned char *xb = nullptr;
    if constexpr (U8) {
        unsigned char *p = bbuf.get() + xoff;
        for (long i = 0; i < 2 * n_in; ++i) { st = st * 1664525u + 1013904223u; p[i] = (unsigned char)(st >> 24); }
        xb = p;
        x = p;
    } else {
        float2 *p = xbuf.data();
        if ((((uintptr_t)p & 15) != 0) != (xoff != 0)) ++p;
        for (long i = 0; i < n_in; ++i) { p[i].x = value(st); p[i].y = value(st); }
        xc = p;
        x = p;
    }
    const bool vec_in = ((uintptr_t)x & (U8 ? 3 : 15)) == 0;
    if (U8 ? (int)((uintptr_t)x & 3) != xoff : vec_in != (xoff == 0)) { ++failures; std::printf("FAIL: the emulator's own stream alignment\n"); return; }

    const std::vector<float2> m = mixed(xc, xb, n_in, tab, first);
    std::vector<float2> want((size_t)n_out);
    for (long i = 0; i < n_out; ++i)
        want[(size_t)i] = written ? contract<FUSED>(m.data(), h.data(), K, U, D, i) : contract_strided<FUSED>(m.data(), h.data(), K, U, D, i);
    if (written)
        for (long i = 0; i < n_out; ++i)
            if (!same(want[(size_t)i], contract_strided<FUSED>(m.data(), h.data(), K, U, D, i))) { ++failures; std::printf("FAIL: the two written forms of the contract differ\n"); return; }

    const int route = upfirdn_route(K, U, D), R = upfirdn_r(K, U, D);
    const unsigned first_mod = ddc_first_mod(first, tab.L);
    int bad = 0, wrong = 0;
    Fenced<float2> ybuf((size_t)n_out + 4);
    float2 *y = ybuf.data();
    if ((((uintptr_t)y & 15) != 0) != (yoff != 0)) ++y;
    const bool yal = ((uintptr_t)y & 15) == 0;
    const long ylead = y - ybuf.data();
    auto untouched = [&] { // nothing but the n_out outputs was written: the fences and the slack around y
        for (long i = 0; i < (long)ybuf.n; ++i)
            if ((i < ylead || i >= ylead + n_out) && !std::isnan(*(const float *)&ybuf.data()[i])) return false;
        return ybuf.intact();
    };
    if (route == 1) {
        const DdcTile<U8> in = {x, n_in, first_mod, tab.dev.data(), tab.L, vec_in ? 1 : 0};
        const float *taps = tbuf.data();
        tile_dispatch_d(Dp, 0, [&](auto d) {
            tiled_r<U8, decltype(d)::value, FUSED>(R, in, ph.data(), taps, (int)Up, (int)Wp, y, n_out, yal, &bad);
            return 0;
        });
        for (long i = 0; i < n_out; ++i) wrong += !same(y[i], want[(size_t)i]);
        if (!untouched()) ++bad;
    }
    // the direct kernel's thread function, every output
    for (auto &v : ybuf.all) v = nan_of(float2{});
    for (long i = 0; i < n_out; ++i) y[i] = ddc_upfirdn_direct_output<U8, FUSED>(x, i, Up, Dp, ph.data(), tbuf.data(), first_mod, tab.dev.data(), tab.L);
    for (long i = 0; i < n_out; ++i) wrong += !same(y[i], want[(size_t)i]);
    if (!untouched()) ++bad;
    if (!tbuf.intact() || !tab.dev.intact() || !xbuf.intact()) ++bad;
    if (bad || wrong) {
        ++failures;
        std::printf("FAIL K %ld U %ld D %ld n %ld %s %s route %d R %d L %u first %llu xoff %d yoff %d: %d wrong outputs, %d fence or bounds violations\n", K, U,
                    D, n_in, U8 ? "u8" : "cf32", FUSED ? "fused" : "exact", route, R, tab.L, first, xoff, yoff, wrong, bad);
    }
}

std::vector<Table> &tables()
{
    static std::vector<Table> t;
    if (t.empty())
        for (unsigned L : {1u, 2u, 3u, 24u, 65536u}) t.emplace_back(L);
    return t;
}

template <bool U8, bool FUSED>
void sweep(long K, long U, long D, long n_in, unsigned &seed, int &turn)
{
    bool written = true; // the K-step form of the contract once per call shape, the strided form for the rest
    for (Table &t : tables()) {
        const unsigned long long firsts[5] = {0ull, 1ull, (unsigned long long)t.L - 1, (1ull << 32) + 5, ~0ull - (unsigned long long)n_in};
        for (unsigned long long first : firsts) {
            // alignments in turn: every (stream offset, output offset) pair comes up many times per shape
            const int nx = U8 ? 4 : 2, xoff = turn % nx, yoff = (turn / nx) % 2;
            ++turn;
            one_call<U8, FUSED>(K, U, D, n_in, t, first, xoff, yoff, seed++, written);
            written = false;
        }
    }
}

void shape(long U, long D, long K, int want_route)
{
    const int route = upfirdn_route(K, U, D);
    if (route != want_route) { ++failures; std::printf("FAIL K %ld U %ld D %ld: route %d, expected %d\n", K, U, D, route, want_route); return; }
    const long Up = upfirdn_period_out(U, D);
    const long T = route == 1 ? 256L * upfirdn_r(K, U, D) * Up : 256;
    unsigned seed = (unsigned)(K * 7919 + U * 104729 + D);
    int turn = 0;
    // outputs just under, at and just over one tile, and a last partial tile behind two whole ones
    for (long n_out : {T - 1, T, T + 1, 2 * T + 37}) {
        const long n_in = ((n_out - 1) * D + K + U - 1) / U; // the shortest input with n_out outputs
        sweep<false, false>(K, U, D, n_in, seed, turn);
        sweep<false, true>(K, U, D, n_in, seed, turn);
        sweep<true, false>(K, U, D, n_in, seed, turn);
        sweep<true, true>(K, U, D, n_in, seed, turn);
        ++turn; // the next count begins on another alignment
    }
}

// one whole tile and a partial one behind it, at a tap count whose tile is past everything shape() stages: the longest table reads
void long_shape(long U, long D, long K, int want_r)
{
    const int route = upfirdn_route(K, U, D), R = upfirdn_r(K, U, D);
    if (route != 1 || R != want_r) { ++failures; std::printf("FAIL K %ld U %ld D %ld: route %d R %d, expected 1 and %d\n", K, U, D, route, R, want_r); return; }
    const long lds = upfirdn_lds_elems(R, upfirdn_period_out(U, D), upfirdn_period_in(U, D), upfirdn_window(K, U, D)) * 8;
    if (lds <= UPFIRDN_LDS_WANT || lds > UPFIRDN_LDS_MAX) { ++failures; std::printf("FAIL K %ld U %ld D %ld: a tile of %ld bytes\n", K, U, D, lds); return; }
    const long n_out = 256L * R * upfirdn_period_out(U, D) + 37;
    const long n_in = ((n_out - 1) * D + K + U - 1) / U;
    unsigned seed = (unsigned)(K * 7919 + U * 104729 + D);
    Table &odd = tables()[2], &big = tables()[4]; // periods 3 and 65536
    one_call<false, false>(K, U, D, n_in, big, (1ull << 32) + 5, 0, 0, seed++, false);
    one_call<false, true>(K, U, D, n_in, odd, 2, 1, 1, seed++, false);
    one_call<true, false>(K, U, D, n_in, odd, ~0ull - (unsigned long long)n_in, 0, 1, seed++, false);
    one_call<true, true>(K, U, D, n_in, big, 65535, 3, 0, seed++, false);
}
} // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "--long")) {
        // the second pass of upfirdn_r at every R (tiles of 52 to 150 KiB: tests/emu_upfirdn --long's list), and the last tap counts
        // route 1 takes at 2/1 and 3/8
        long_shape(2, 1, 11776, 4);
        long_shape(3, 2, 36864, 2);
        long_shape(2, 1, 25396, 1);
        long_shape(2, 1, 36863, 1);
        long_shape(3, 8, 43013, 1);
    } else if (argc >= 2) {
        return 2;
    } else {
        const long r1[][3] = {{2, 1, 63}, {3, 2, 64}, {2, 3, 31}, {4, 5, 100}, {3, 8, 17}, {7, 10, 40}, {6, 4, 50}, {5, 1, 3}, {1, 5, 127}};
        for (auto &s : r1) shape(s[0], s[1], s[2], 1);
        const long r2[][3] = {{160, 147, 481}, {3, 16, 33}, {2, 7, 9}};
        for (auto &s : r2) shape(s[0], s[1], s[2], 2);
    }
    if (failures) { std::printf("emu_ddc_upfirdn: %d failures in %ld calls\n", failures, calls); return 1; }
    std::printf("emu_ddc_upfirdn ok (%ld calls)\n", calls);
    return 0;
}
