// The fused 2048-point real overlap-save block (libredio_amd/csrc/ovsave_real_kernels.hip) run on the CPU, sixty-four lanes one at a
// time in the kernel's own phases: the one-wave transform's passes (fft_core.h), Z in natural order in the wave's image, the
// register-output forward split and the inverse split's hand-over (fftr_core.h), the product and the masked pair store
// (ovsave_real_core.h).  A phase ends where the kernel has a wave_lds_fence(): every lane finishes it before any lane goes on.
#include "../../libredio_amd/csrc/fft_core.h"
#include "../../libredio_amd/csrc/ovsave_real_core.h"
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

std::vector<float2> make_tw(int n, int inverse)
{
    std::vector<float2> tw((size_t)n);
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
    for (int i = 0; i < n; ++i) {
        double phase = -2 * pi * i / n;
        if (inverse) phase *= -1;
        tw[i] = make_float2((float)cos(phase), (float)sin(phase));
    }
    return tw;
}

// fft1k_wave_stages0to3 + fft1k_passC: v[lane][t] = x[lane + 64 t] on entry, v[lane][4 q + j] = X[lane + 64 q + 256 j] on return
template <bool INV>
void wave_fft(float2 (*v)[16])
{
    const std::vector<float2> tw = make_tw(1024, INV);
    std::vector<float2> ex(FFT1K_LDS), ex2(FFT1K_LDS);
    for (int lane = 0; lane < 64; ++lane) {
        fft1k_passA<INV>(v[lane], tw.data());
        for (int k4 = 0; k4 < 4; ++k4)
            for (int k3 = 0; k3 < 4; ++k3) ex[fft1k_A_store(lane, k3, k4)] = v[lane][k3 + 4 * k4];
    }
    for (int lane = 0; lane < 64; ++lane) {
        for (int e = 0; e < 16; ++e) v[lane][e] = ex[fft1k_B_load(lane, e)];
        Fft1kTw t;
        fft1k_load_tw(t, lane, tw.data());
        fft1k_passB<INV>(v[lane], t);
        for (int k2 = 0; k2 < 4; ++k2)
            for (int k1 = 0; k1 < 4; ++k1) ex2[fft1k_B_store(lane, k1, k2)] = v[lane][k1 + 4 * k2];
    }
    for (int lane = 0; lane < 64; ++lane) {
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 4; ++j) v[lane][4 * q + j] = ex2[fft1k_C_load(lane, q, j)];
        Fft1kTw t;
        fft1k_load_tw(t, lane, tw.data());
        fft1k_passC<INV>(v[lane], t);
    }
}
} // namespace

// One block.  x: 2048 samples; Hc: 1025 bins; hop: even, 2 ... 2048; out: 2048 floats, of which the first hop are written.
// freq / prod (1025 bins each): the split's and the product's registers, for the caller to compare; stores (1024): writes per
// output pair.  Returns 1 when the hand-over wrote each of the image's slots 512 ... 1023 exactly once.
extern "C" int emu_ovsave_real2k_block(const float *x, const float2 *Hc, long hop, float *out, float2 *freq, float2 *prod, int *stores)
{
    static float2 v[64][16];
    const float2 *row = reinterpret_cast<const float2 *>(x);
    for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 16; ++i) v[lane][i] = row[lane + 64 * i];
    wave_fft<false>(v);
    std::vector<float2> ex(FFT1K_LDS);
    for (int lane = 0; lane < 64; ++lane)
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 4; ++j) ex[lane + 64 * q + 256 * j] = v[lane][4 * q + j];
    std::vector<float2> stw_f(FFTR1K_M / 2), stw_i(FFTR1K_M / 2);
    fftr_super_tw(FFTR1K_M, 0, stw_f.data());
    fftr_super_tw(FFTR1K_M, 1, stw_i.data());
    static float2 a[64][8], c[64][8], mid[64];
    for (int lane = 63; lane >= 0; --lane) { // every lane reads its partner Z before the image is overwritten
        Fftr1kTw w;
        fftr1k_load_tw(w, lane, stw_f.data());
        fftr1k_post_lane_regs(v[lane], ex.data(), w, lane, a[lane], c[lane], mid[lane]);
        for (int t = 0; t < 8; ++t) {
            freq[lane + 64 * t] = a[lane][t];
            freq[fftr1k_partner(lane, t)] = c[lane][t];
        }
        if (lane == 0) freq[FFTR1K_M / 2] = mid[0];
        ovsr1k_product(a[lane], c[lane], mid[lane], Hc, lane);
        for (int t = 0; t < 8; ++t) {
            prod[lane + 64 * t] = a[lane][t];
            prod[fftr1k_partner(lane, t)] = c[lane][t];
        }
        if (lane == 0) prod[FFTR1K_M / 2] = mid[0];
    }
    std::vector<int> n(FFT1K_LDS, 0);
    for (int lane = 0; lane < 64; ++lane) {
        Fftr1kTw w;
        fftr1k_load_tw(w, lane, stw_i.data());
        fftr1k_pre_lane(a[lane], c[lane], mid[lane], w, lane, v[lane], Counted{ex.data(), n.data()});
    }
    int ok = 1;
    for (int i = 0; i < FFT1K_LDS; ++i) ok &= n[i] == ((i >= FFTR1K_M / 2 && i < FFTR1K_M) ? 1 : 0);
    for (int lane = 0; lane < 64; ++lane) fftr1k_pre_gather(v[lane], ex.data(), lane);
    wave_fft<true>(v);
    const float scale = 1.0f / 2048.0f;
    for (int lane = 0; lane < 64; ++lane) ovsr1k_store(v[lane], Counted{reinterpret_cast<float2 *>(out), stores}, lane, hop, scale);
    return ok;
}
