// The fused 1024-point power-spectrum kernel on u8 I/Q bytes (libredio_amd/csrc/pspec_kernels.hip, pspec1k_u8_kernel) run on the CPU,
// sixty-four lanes one at a time in the kernel's own phases: load of the raw 16-bit words, convert (i2f), window, the one-wave
// transform's passes (fft_core.h), square and accumulate, the segment and row folds, the store (pspec_core.h).  The raw words of
// transform i + 1 are loaded while transform i is in flight, as the kernel prefetches them.  A phase ends where the kernel has a
// wave_lds_fence(): every lane finishes it before any lane goes on.  Then the generic path's gather from bytes, and the conversion alone.
#include "../../libredio_amd/csrc/fft_core.h"
#include "../../libredio_amd/csrc/pspec_core.h"
#include <vector>

using namespace redio;

namespace {
// a destination that counts the writes each element receives
struct Counted {
    float *p;
    int *n;
    struct Ref {
        float *q;
        int *c;
        void operator=(float v) const { *q = v; ++*c; }
    };
    Ref operator[](long i) const { return Ref{p + i, n + i}; }
};

// the byte stream seen as the kernel sees it: one little-endian 16-bit word per sample, at any 2-byte boundary
struct Words {
    const uint8_t *b;
    uint16_t operator[](long i) const { return (uint16_t)(b[2 * i] | (b[2 * i + 1] << 8)); }
    Words operator+(long i) const { return Words{b + 2 * i}; }
};

std::vector<float2> make_tw(int n)
{
    std::vector<float2> tw((size_t)n);
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
    for (int i = 0; i < n; ++i) {
        const double phase = -2 * pi * i / n;
        tw[i] = make_float2((float)cos(phase), (float)sin(phase));
    }
    return tw;
}

// fft1k_wave_stages0to3 + fft1k_passC: v[lane][t] = x[lane + 64 t] on entry, v[lane][4 q + j] = X[lane + 64 q + 256 j] on return
void wave_fft(float2 (*v)[16], const std::vector<float2> &tw)
{
    std::vector<float2> ex(FFT1K_LDS), ex2(FFT1K_LDS);
    for (int lane = 0; lane < 64; ++lane) {
        fft1k_passA<false>(v[lane], tw.data());
        for (int k4 = 0; k4 < 4; ++k4)
            for (int k3 = 0; k3 < 4; ++k3) ex[fft1k_A_store(lane, k3, k4)] = v[lane][k3 + 4 * k4];
    }
    for (int lane = 0; lane < 64; ++lane) {
        for (int e = 0; e < 16; ++e) v[lane][e] = ex[fft1k_B_load(lane, e)];
        Fft1kTw t;
        fft1k_load_tw(t, lane, tw.data());
        fft1k_passB<false>(v[lane], t);
        for (int k2 = 0; k2 < 4; ++k2)
            for (int k1 = 0; k1 < 4; ++k1) ex2[fft1k_B_store(lane, k1, k2)] = v[lane][k1 + 4 * k2];
    }
    for (int lane = 0; lane < 64; ++lane) {
        for (int q = 0; q < 4; ++q)
            for (int j = 0; j < 4; ++j) v[lane][4 * q + j] = ex2[fft1k_C_load(lane, q, j)];
        Fft1kTw t;
        fft1k_load_tw(t, lane, tw.data());
        fft1k_passC<false>(v[lane], t);
    }
}
} // namespace

// One launch of pspec1k_u8_kernel: nunits units (rows, or with `split` segments) of the byte stream; win: 1024 values or null; dst:
// 1024 f32 per unit; stores: writes per element of dst.
extern "C" void emu_pspec1k_u8(const uint8_t *bytes, long step, long K, const float *win, int split, long nunits, float *dst, int *stores)
{
    const std::vector<float2> tw = make_tw(1024);
    const Words x{bytes};
    static uint16_t raw[64][16];
    static float2 v[64][16];
    static float w[64][16], seg[64][16], row[64][16];
    for (long u = 0; u < nunits; ++u) {
        long g0, cnt;
        pspec_unit(u, K, split != 0, g0, cnt);
        if (win)
            for (int lane = 0; lane < 64; ++lane) pspec1k_load_window(w[lane], win, lane);
        Words p = x + g0 * step;
        for (int lane = 0; lane < 64; ++lane) pspec1k_load_raw(raw[lane], p, lane);
        for (long i = 0; i < cnt; ++i) {
            const Words pn = (i + 1 < cnt) ? p + step : p;
            for (int lane = 0; lane < 64; ++lane) {
                pspec1k_convert(v[lane], raw[lane]);
                pspec1k_load_raw(raw[lane], pn, lane);
                if (win) pspec1k_window(v[lane], w[lane]);
            }
            wave_fft(v, tw);
            const PspecStep s = pspec_step(i, cnt);
            for (int lane = 0; lane < 64; ++lane) {
                pspec1k_accum(v[lane], seg[lane], s.seg_first);
                if (s.seg_last) pspec1k_fold(seg[lane], row[lane], s.row_first);
            }
            p = pn;
        }
        for (int lane = 0; lane < 64; ++lane) pspec1k_store(row[lane], Counted{dst + u * 1024, stores + u * 1024}, lane);
    }
}

// pspec_rows_u8_kernel's lane steps: ntr rows of N samples that start every `step` samples of the byte stream, two consecutive
// elements of the packed rows per step and the last element of an odd count on its own; stores: writes per element
extern "C" void emu_pspec_rows_u8(const uint8_t *bytes, const float *win, long ntr, long N, long step, float2 *rows, int *stores)
{
    const Words x{bytes};
    const unsigned total = (unsigned)(ntr * N);
    for (unsigned q = 0; q < total / 2; ++q) {
        float2 v0, v1;
        pspec_rows_u8_pair(x, win, win != nullptr, q, (unsigned)N, step, v0, v1);
        rows[2 * q] = v0;
        rows[2 * q + 1] = v1;
        ++stores[2 * q];
        ++stores[2 * q + 1];
    }
    if (total & 1) {
        const unsigned i = total - 1, b = i / (unsigned)N;
        rows[i] = pspec_rows_u8_thread(x, win, win != nullptr, (long)b, (long)(i - b * (unsigned)N), step);
        ++stores[i];
    }
}

// i2f on every byte value: out[b] = the kernels' conversion of byte b
extern "C" void emu_i2f_all(float *out)
{
    for (unsigned b = 0; b < 256; ++b) out[b] = i2f(b);
}
