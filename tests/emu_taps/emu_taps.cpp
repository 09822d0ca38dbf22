// The host path of the two FIR lane programs of the chain kernels, run lane by lane over an image laid out as the kernels lay it out
// (FirGeomV::lds_index): fir_lane_v (taps staged per chunk, any taps) and fir_lane_v_res (bit-palindromic taps held as ceil(K/2)
// values).  x: (lanes * 4 - 1) * D + K cf32 samples; out_*: lanes * 4 cf32 outputs, output o = fold over j of x[o * D + j] * taps[j].
#include "../../libredio_amd/csrc/fir_core.h"
#include <string.h>
#include <vector>

using namespace redio;

template <int K, int D, bool FUSED>
static int run(const float *x, const float *taps, int lanes, float *out_staged, float *out_res)
{
    constexpr int R = 4;
    using G = FirGeomV<K, D, R>;
    const int n = G::tile_in(lanes * R);
    std::vector<float4> img(G::lds_elems(lanes * R) / 2 + 2, make_float4(0, 0, 0, 0));
    float2 *e = reinterpret_cast<float2 *>(img.data());
    for (int i = 0; i < n; ++i) e[G::lds_index(i)] = make_float2(x[2 * i], x[2 * i + 1]);
    std::vector<float> h(taps, taps + K);
    h.resize(K + 16, 0.0f);
    FirTapsResident<K> t;
    fir_taps_resident_load(t, h.data());
    for (int lane = 0; lane < lanes; ++lane) {
        float2 a[R], b[R];
        for (int r = 0; r < R; ++r) a[r] = b[r] = make_float2(0.f, 0.f);
        fir_lane_v<K, D, R, FUSED, 8>(img.data(), lane, h.data(), a);
        fir_lane_v_res<K, D, R, FUSED, 8>(img.data(), lane, t, b);
        memcpy(out_staged + 2 * R * lane, a, sizeof(a));
        memcpy(out_res + 2 * R * lane, b, sizeof(b));
    }
    return 0;
}

extern "C" int emu_taps_fir(int K, int D, int fused, const float *x, const float *taps, int lanes, float *out_staged, float *out_res)
{
#define CASE(k, d)                                                                                 \
    if (K == k && D == d) return fused ? run<k, d, true>(x, taps, lanes, out_staged, out_res) : run<k, d, false>(x, taps, lanes, out_staged, out_res)
    CASE(127, 5);
    CASE(63, 5);
    CASE(127, 3);
    CASE(127, 1);
    CASE(63, 1);
    CASE(64, 2); // an even tap count: no middle tap
    CASE(7, 2);  // a window shorter than a chunk
#undef CASE
    return -1;
}
