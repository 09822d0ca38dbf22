// The split step of the real-input transform (libredio_amd/csrc/fftr_core.h) run on the CPU one thread / one lane at a time, over a
// complex transform computed elsewhere (the oracle): validates the arithmetic and the index maps without a GPU.
#include "../../libredio_amd/csrc/fftr_core.h"
#include <vector>

using namespace redio;

namespace {
// a destination that counts the writes each element receives
struct Counted {
    float2 *p;
    int *n;
    struct Ref {
        float2 *q;
        int *c;
        void operator=(float2 v) const { *q = v; ++*c; }
    };
    Ref operator[](long i) const { return Ref{p + i, n + i}; }
};
bool all_once(const std::vector<int> &n, size_t lo, size_t hi)
{
    for (size_t i = lo; i < hi; ++i)
        if (n[i] != 1) return false;
    return true;
}
} // namespace

extern "C" void emu_fftr_super_tw(int M, int inverse, float2 *tw) { fftr_super_tw(M, inverse, tw); }

// the generic kernels' thread programs, threads in descending order (any order gives the same result); src: Z (M) or freq (M + 1).
// Returns 1 when every output element was written exactly once.
extern "C" int emu_fftr_split(int M, int inverse, const float2 *src, float2 *dst)
{
    std::vector<float2> stw((size_t)(M / 2 > 0 ? M / 2 : 1));
    fftr_super_tw(M, inverse, stw.data());
    const size_t nout = inverse ? (size_t)M : (size_t)M + 1;
    std::vector<int> n(nout, 0);
    for (int j = M / 2; j >= 0; --j) {
        if (inverse) fftr_pre_thread(j, M, src, Counted{dst, n.data()}, stw.data());
        else fftr_post_thread(j, M, src, Counted{dst, n.data()}, stw.data());
    }
    return all_once(n, 0, nout) ? 1 : 0;
}

// the fused forward kernel's split: every lane holds the transform's result in the register layout fft1k_wave_regs leaves
// (v[4 q + j] = Z[lane + 64 q + 256 j]) and reads its partners from the natural-order image
extern "C" int emu_fftr1k_post(const float2 *Z, float2 *freq)
{
    std::vector<float2> stw(FFTR1K_M / 2);
    fftr_super_tw(FFTR1K_M, 0, stw.data());
    std::vector<int> n(FFTR1K_M + 1, 0);
    for (int lane = 63; lane >= 0; --lane) {
        float2 v[16];
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 4; ++j) v[4 * q + j] = Z[lane + 64 * q + 256 * j];
        Fftr1kTw w;
        fftr1k_load_tw(w, lane, stw.data());
        fftr1k_post_lane(v, Z, w, lane, Counted{freq, n.data()});
    }
    return all_once(n, 0, FFTR1K_M + 1) ? 1 : 0;
}

// the fused inverse kernel's split: loads, pair steps, the hand-over through the image, the gather; T[lane + 64 t] = input register t
extern "C" int emu_fftr1k_pre(const float2 *freq, float2 *T)
{
    std::vector<float2> stw(FFTR1K_M / 2);
    fftr_super_tw(FFTR1K_M, 1, stw.data());
    std::vector<float2> ex(FFTR1K_M);
    std::vector<int> n(FFTR1K_M, 0);
    float2 v[64][16];
    for (int lane = 0; lane < 64; ++lane) {
        float2 a[8], b[8], mid;
        fftr1k_load_row(freq, lane, a, b, mid);
        Fftr1kTw w;
        fftr1k_load_tw(w, lane, stw.data());
        fftr1k_pre_lane(a, b, mid, w, lane, v[lane], Counted{ex.data(), n.data()});
    }
    if (!all_once(n, FFTR1K_M / 2, FFTR1K_M)) return 0;
    for (int lane = 0; lane < 64; ++lane) {
        fftr1k_pre_gather(v[lane], ex.data(), lane);
        for (int t = 0; t < 16; ++t) T[lane + 64 * t] = v[lane][t];
    }
    return 1;
}

// the index map on its own: for lane != 0 the partner of lane's step t is lane 64 - lane's register fftr1k_reg(15 - t)
extern "C" int emu_fftr1k_map_ok(void)
{
    for (int lane = 0; lane < 64; ++lane)
        for (int t = 0; t < 8; ++t) {
            const int k = lane + 64 * t, p = fftr1k_partner(lane, t);
            if (p != FFTR1K_M - k) return 0;
            if (lane != 0 && p != (64 - lane) + 64 * (15 - t)) return 0;
            if (lane == 0 && t != 0 && p != 64 * (16 - t)) return 0;
        }
    for (int t = 0; t < 16; ++t) { // register 4 q + j holds X[lane + 64 (q + 4 j)]
        const int r = fftr1k_reg(t), q = r >> 2, j = r & 3;
        if (q + 4 * j != t) return 0;
    }
    return 1;
}
