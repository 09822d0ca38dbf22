// emu_upfirdn.cpp -- CPU emulation of the rational resampler's kernels (libredio_amd/csrc/upfirdn_kernels.hip): every thread of every
// workgroup of a call runs route 1's loader, phase loop and store loop -- the very sources the device compiles (upfirdn_core.h) --
// against fenced copies of the stream, the polyphase taps, the LDS allocation and the output; the direct kernel's per-thread function
// runs on the same calls.  Outputs are compared bit for bit with the contract written out (include/redio.h: the fold over j, stuffed
// zeros skipped), and every fence must be intact.  The LDS image and the output tile behind it have exactly upfirdn_img_elems and
// 256 R U' elements (together upfirdn_lds_elems), each between fences of NaN 8192 elements wide: a lane that reads past the image
// computes NaN, one that writes past either is found afterwards.
// A stand-alone program: exit status 0 and "emu_upfirdn ok" when everything held.
//   emu_upfirdn                       the shapes of tests/test_gpu_upfirdn.py, four output counts around the tile each
//   emu_upfirdn --long                long filters: the tiles of 52 to 150 KiB and the last tap counts of route 1, one whole and one
//                                     partial tile each
//   emu_upfirdn --geometry U D K ...  one line "U D K route R lds_elems window" per triple: the headers' own geometry
#include "../../libredio_amd/csrc/upfirdn_core.h"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace redio;

namespace {
constexpr int FENCE = 64;       // elements in front of and behind every buffer
constexpr int LDS_FENCE = 8192; // and around the two parts of the LDS allocation: wider than any window's stride past the image
int failures = 0;

float value(unsigned &state)
{
    state = state * 1664525u + 1013904223u;
    return (float)(int)(state >> 8) * (1.0f / 8388608.0f) - 1.0f;
}
void fill(float &v, unsigned &st) { v = value(st); }
void fill(float2 &v, unsigned &st) { v.x = value(st); v.y = value(st); }
float2 nan_of(float2) { return make_float2(NAN, NAN); }
float nan_of(float) { return NAN; }
bool same(const float &a, const float &b) { return std::memcmp(&a, &b, 4) == 0; }
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

// the contract, written out
template <typename T, bool FUSED>
T contract(const T *x, const float *h, long K, long U, long D, long i)
{
    T acc{};
    for (long j = 0; j < K; ++j)
        if ((i * D + j) % U == 0) acc = mac<FUSED>(x[(i * D + j) / U], h[j], acc);
    return acc;
}

// the same fold for long filters: the first j that meets a sample, then every U-th
template <typename T, bool FUSED>
T contract_strided(const T *x, const float *h, long K, long U, long D, long i)
{
    T acc{};
    for (long j = (U - (i * D) % U) % U; j < K; j += U) acc = mac<FUSED>(x[(i * D + j) / U], h[j], acc);
    return acc;
}

template <typename T, int DP, int R, bool FUSED>
void tiled_call(const T *x, long n_in, const UpfirdnPhase *ph, const float *taps, int Up, int Wp, T *y, long n_out, bool vec_in, bool vec_out, int *bad)
{
    constexpr int NT = 256, NQ = NT * R, LSTR = R * DP;
    constexpr bool STREAM = DP >= 2;
    const long img = upfirdn_img_elems(R, DP, Wp), lds = upfirdn_lds_elems(R, Up, DP, Wp);
    const long per_tile = (long)NQ * Up;
    if (lds - img != per_tile || lds * 8 > UPFIRDN_LDS_MAX) ++*bad; // the launch's allocation is the image and the output tile, and fits
    for (long t = 0; t < (n_out + per_tile - 1) / per_tile; ++t) {
        Fenced<T> image((size_t)img, LDS_FENCE), tile((size_t)(lds - img), LDS_FENCE);
        T *xs = image.data(), *ys = tile.data();
        const long in0 = t * NQ * DP;
        for (int tid = 0; tid < NT; ++tid)
            upfirdn_load_thread<T, STREAM>(tid, NT, x + in0, n_in - in0, (int)upfirdn_tile_in(R, DP, Wp), vec_in, [&](int n, T v) {
                const long at = tile_image_index(n, LSTR);
                if (at < 0 || at >= img) ++*bad; else xs[at] = v;
            });
        for (int tid = 0; tid < NT; ++tid) upfirdn_phases_thread<T, DP, R, FUSED, 16>(xs, ys, tid, ph, taps, Up);
        for (int tid = 0; tid < NT; ++tid) upfirdn_store_thread<T, STREAM>(tid, NT, ys, NQ * Up, y + t * per_tile, n_out - t * per_tile, vec_out);
        if (!image.intact() || !tile.intact()) ++*bad;
    }
}

template <typename T, int DP, bool FUSED>
void tiled_r(int R, const T *x, long n_in, const UpfirdnPhase *ph, const float *taps, int Up, int Wp, T *y, long n_out, bool vi, bool vo, int *bad)
{
    if (R == 4) {
        if constexpr (upfirdn_r_max(DP) >= 4) tiled_call<T, DP, 4, FUSED>(x, n_in, ph, taps, Up, Wp, y, n_out, vi, vo, bad);
        else ++*bad;
    } else if (R == 2) tiled_call<T, DP, 2, FUSED>(x, n_in, ph, taps, Up, Wp, y, n_out, vi, vo, bad);
    else tiled_call<T, DP, 1, FUSED>(x, n_in, ph, taps, Up, Wp, y, n_out, vi, vo, bad);
}

// light (long filters): the contract by strides, aligned in and out and both one sample off, the direct form once
template <typename T, bool FUSED>
void one_call(long K, long U, long D, long n_in, unsigned seed, bool light = false)
{
    const long Up = upfirdn_period_out(U, D), Dp = upfirdn_period_in(U, D), Wp = upfirdn_window(K, U, D);
    const long n_out = (long)upfirdn_nout(n_in, K, U, D);
    unsigned st = seed;
    std::vector<float> h((size_t)K);
    for (float &v : h) fill(v, st);
    // the stream one sample off a 16-byte boundary for the scalar paths, on one for the wide ones
    Fenced<T> xbuf((size_t)n_in + 4);
    std::vector<UpfirdnPhase> ph;
    std::vector<float> tp;
    upfirdn_build(h.data(), K, U, D, ph, tp);
    Fenced<float> tbuf(tp.size());
    std::memcpy(tbuf.data(), tp.data(), tp.size() * sizeof(float));
    std::vector<T> want((size_t)n_out);
    const int route = upfirdn_route(K, U, D), R = upfirdn_r(K, U, D);
    int bad = 0, wrong = 0;
    for (int off = 0; off < 2; ++off) {
        // x: `off` samples behind the buffer's start; the fence is re-laid around exactly n_in samples so that a read past the end is NaN
        for (auto &v : xbuf.all) v = nan_of(T{});
        T *x = xbuf.data() + off;
        unsigned sx = seed ^ 0x9E3779B9u;
        for (long i = 0; i < n_in; ++i) fill(x[i], sx);
        if (off == 0)
            for (long i = 0; i < n_out; ++i)
                want[(size_t)i] = light ? contract_strided<T, FUSED>(x, h.data(), K, U, D, i) : contract<T, FUSED>(x, h.data(), K, U, D, i);
        const bool aligned = ((uintptr_t)x & 15) == 0;
        Fenced<T> ybuf((size_t)n_out + 4);
        for (int yoff = 0; yoff < 2; ++yoff) {
            if (light && yoff != off) continue;
            T *y = ybuf.data() + yoff;
            const bool yal = ((uintptr_t)y & 15) == 0;
            auto untouched = [&] { // nothing but the n_out outputs was written: the fences and the slack around y
                for (long i = 0; i < (long)ybuf.n; ++i)
                    if ((i < yoff || i >= yoff + n_out) && !std::isnan(*(const float *)&ybuf.data()[i])) return false;
                return ybuf.intact();
            };
            if (route == 1) {
                for (auto &v : ybuf.all) v = nan_of(T{});
                const float *taps = tbuf.data();
                tile_dispatch_d(Dp, 0, [&](auto d) {
                    tiled_r<T, decltype(d)::value, FUSED>(R, x, n_in, ph.data(), taps, (int)Up, (int)Wp, y, n_out, aligned, yal, &bad);
                    return 0;
                });
                for (long i = 0; i < n_out; ++i) wrong += !same(y[i], want[(size_t)i]);
                if (!untouched()) ++bad;
            }
            // the direct kernel's thread function, every output
            if (light && off) continue;
            for (auto &v : ybuf.all) v = nan_of(T{});
            for (long i = 0; i < n_out; ++i) y[i] = upfirdn_direct_output<T, FUSED>(x, i, Up, Dp, ph.data(), tbuf.data());
            for (long i = 0; i < n_out; ++i) wrong += !same(y[i], want[(size_t)i]);
            if (!untouched()) ++bad;
        }
    }
    if (!tbuf.intact()) ++bad;
    if (bad || wrong) {
        ++failures;
        std::printf("FAIL K %ld U %ld D %ld n %ld %s %s route %d R %d: %d wrong outputs, %d fence or bounds violations\n", K, U, D, n_in,
                    sizeof(T) == 8 ? "cf32" : "f32", FUSED ? "fused" : "exact", route, R, wrong, bad);
    }
}

void shape(long U, long D, long K, int want_route)
{
    const int route = upfirdn_route(K, U, D);
    if (route != want_route) { ++failures; std::printf("FAIL K %ld U %ld D %ld: route %d, expected %d\n", K, U, D, route, want_route); return; }
    const long Up = upfirdn_period_out(U, D);
    const long T = route == 1 ? 256L * upfirdn_r(K, U, D) * Up : 256;
    unsigned seed = (unsigned)(K * 7919 + U * 104729 + D);
    // outputs just under, at and just over one tile, and a last partial tile behind two whole ones
    for (long n_out : {T - 1, T, T + 1, 2 * T + 37}) {
        const long n_in = ((n_out - 1) * D + K + U - 1) / U; // the shortest input with n_out outputs
        one_call<float, false>(K, U, D, n_in, seed++);
        one_call<float, true>(K, U, D, n_in, seed++);
        one_call<float2, false>(K, U, D, n_in, seed++);
        one_call<float2, true>(K, U, D, n_in, seed++);
    }
}

// one whole tile and a partial one behind it, at a tap count whose tile is past everything shape() stages
void long_shape(long U, long D, long K, int want_route, int want_r)
{
    const int route = upfirdn_route(K, U, D), R = upfirdn_r(K, U, D);
    if (route != want_route || R != want_r) {
        ++failures;
        std::printf("FAIL K %ld U %ld D %ld: route %d R %d, expected %d and %d\n", K, U, D, route, R, want_route, want_r);
        return;
    }
    const long n_out = (route == 1 ? 256L * R * upfirdn_period_out(U, D) : 256) + 37;
    const long n_in = ((n_out - 1) * D + K + U - 1) / U;
    unsigned seed = (unsigned)(K * 7919 + U * 104729 + D);
    one_call<float, false>(K, U, D, n_in, seed++, true);
    one_call<float, true>(K, U, D, n_in, seed++, true);
    one_call<float2, false>(K, U, D, n_in, seed++, true);
    one_call<float2, true>(K, U, D, n_in, seed++, true);
}

int geometry(int argc, char **argv)
{
    if ((argc - 2) % 3 != 0) return 2;
    for (int i = 2; i + 2 < argc; i += 3) {
        const long U = std::atol(argv[i]), D = std::atol(argv[i + 1]), K = std::atol(argv[i + 2]);
        if (U < 1 || D < 1 || K < 1) return 2;
        const int R = upfirdn_r(K, U, D);
        const long Wp = upfirdn_window(K, U, D);
        std::printf("%ld %ld %ld %d %d %ld %ld\n", U, D, K, upfirdn_route(K, U, D), R,
                    R ? upfirdn_lds_elems(R, upfirdn_period_out(U, D), upfirdn_period_in(U, D), Wp) : 0L, Wp);
    }
    return 0;
}
} // namespace

int main(int argc, char **argv)
{
    if (argc >= 2 && !std::strcmp(argv[1], "--geometry")) return geometry(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "--long")) {
        // the second pass of upfirdn_r at every R (tiles of 52 to 150 KiB), then the last tap counts route 1 takes and the first it leaves
        long_shape(2, 1, 11776, 1, 4);
        long_shape(3, 2, 36864, 1, 2);
        long_shape(2, 1, 25396, 1, 1);
        long_shape(2, 1, 36863, 1, 1);
        long_shape(3, 8, 43013, 1, 1);
        long_shape(2, 1, 36864, 2, 0);
        long_shape(3, 8, 43014, 2, 0);
        if (failures) { std::printf("emu_upfirdn: %d failures\n", failures); return 1; }
        std::printf("emu_upfirdn ok\n");
        return 0;
    }
    if (argc >= 2) return 2;
    // route 1: the shapes of tests/test_gpu_upfirdn.py (gcd 2, phases without taps and U' = 1 among them)
    const long r1[][3] = {{2, 1, 63}, {3, 2, 64}, {2, 3, 31}, {4, 5, 100}, {5, 4, 127}, {16, 1, 255}, {3, 8, 17}, {7, 10, 40}, {6, 4, 50}, {5, 1, 3}, {1, 5, 127}};
    for (auto &s : r1) shape(s[0], s[1], s[2], 1);
    const long r2[][3] = {{160, 147, 481}, {3, 16, 33}, {17, 1, 40}, {2, 7, 9}};
    for (auto &s : r2) shape(s[0], s[1], s[2], 2);
    if (failures) { std::printf("emu_upfirdn: %d failures\n", failures); return 1; }
    std::printf("emu_upfirdn ok\n");
    return 0;
}
