// The fused 2048-point real-input power-spectrum kernel (libredio_amd/csrc/pspec_real_kernels.hip, pspecr2k_kernel) run on the CPU,
// sixty-four lanes one at a time in the kernel's own phases: load (as pairs or as single floats), window, the one-wave transform's
// passes (fft_core.h), the LDS image of Z, the split step squared pair by pair (fftr_core.h), the segment and row folds, the stores
// (pspec_real_core.h).  A phase ends where the kernel has a wave_lds_fence(): every lane finishes it before any lane goes on.  Then
// the generic path's thread programs: the row gather, and the accumulate and fold passes over packed spectra of N / 2 + 1 bins.
#include "../../libredio_amd/csrc/fft_core.h"
#include "../../libredio_amd/csrc/pspec_real_core.h"
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

// One launch of pspecr2k_kernel: nunits units (rows, or with `split` segments) of the real stream x; win: 2048 values or null; pairs:
// the 8-byte load form (x 8-byte aligned and step even, as the launcher checks) or the two-float form; dst: 1025 f32 per unit; stores:
// writes per element of dst.
extern "C" void emu_pspecr2k(const float *x, long step, long K, const float *win, int split, int pairs, long nunits, float *dst, int *stores)
{
    const std::vector<float2> tw = make_tw(FFTR1K_M);
    std::vector<float2> stw(FFTR1K_M / 2);
    fftr_super_tw(FFTR1K_M, 0, stw.data());
    static float2 v[64][16], w[64][16];
    static float p[64][17], seg[64][17], row[64][17];
    std::vector<float2> ex(FFT1K_LDS);
    for (long u = 0; u < nunits; ++u) {
        long g0, cnt;
        pspec_unit(u, K, split != 0, g0, cnt);
        if (win)
            for (int lane = 0; lane < 64; ++lane) pspecr2k_load_window(w[lane], win, lane);
        for (long i = 0; i < cnt; ++i) {
            const float *q = x + (g0 + i) * step;
            for (int lane = 0; lane < 64; ++lane) {
                if (pairs) pspecr2k_load_pairs(v[lane], reinterpret_cast<const float2 *>(q), lane);
                else pspecr2k_load_singles(v[lane], q, lane);
                if (win) pspecr2k_window(v[lane], w[lane]);
            }
            wave_fft(v, tw);
            for (int lane = 0; lane < 64; ++lane) pspecr2k_image(v[lane], ex.data(), lane);
            const PspecStep s = pspec_step(i, cnt);
            for (int lane = 0; lane < 64; ++lane) {
                Fftr1kTw sw;
                fftr1k_load_tw(sw, lane, stw.data());
                pspecr2k_split_power(v[lane], ex.data(), sw, lane, p[lane]);
                pspecr2k_accum(p[lane], seg[lane], s.seg_first);
                if (s.seg_last) pspecr2k_fold(seg[lane], row[lane], s.row_first);
            }
        }
        for (int lane = 0; lane < 64; ++lane) pspecr2k_store(row[lane], Counted{dst + u * PSPECR2K_B, stores + u * PSPECR2K_B}, lane);
    }
}

// pspec_real_rows_kernel's threads: ntr packed rows of N f32 gathered from x every `step` samples, times the window when there is one
extern "C" void emu_pspec_real_rows(const float *x, const float *win, long ntr, long N, long step, float *rows, int *stores)
{
    for (long i = 0; i < ntr * N; ++i) {
        const long b = i / N, n = i - b * N;
        rows[i] = pspec_real_rows_thread(x, win, win != nullptr, b, n, step);
        ++stores[i];
    }
}

// pspec_accum_kernel's threads over every segment of nrows rows of K packed spectra of B = N / 2 + 1 bins (part: B f32 per segment),
// then pspec_fold_kernel's threads (out: B f32 per row), as pspec_api.hip launches them; stores_part / stores_out: writes per element
extern "C" void emu_pspec_real_generic(const float2 *spec, long B, long K, long nrows, float *part, float *out, int *stores_part, int *stores_out)
{
    const long S = pspec_nseg(K);
    for (long q = 0; q < nrows * S; ++q)
        for (long k = 0; k < B; ++k) {
            long g, cnt;
            pspec_segment(q, K, S, g, cnt);
            part[q * B + k] = pspec_accum_thread(spec + g * B, B, cnt, k);
            ++stores_part[q * B + k];
        }
    for (long r = 0; r < nrows; ++r)
        for (long k = 0; k < B; ++k) {
            out[r * B + k] = pspec_fold_thread(part + r * S * B, B, S, k);
            ++stores_out[r * B + k];
        }
}
