// The fused 1024-point power-spectrum kernel (libredio_amd/csrc/pspec_kernels.hip, pspec1k_kernel) run on the CPU, sixty-four lanes
// one at a time in the kernel's own phases: load, window, the one-wave transform's passes (fft_core.h), square and accumulate, the
// segment and row folds, the store (pspec_core.h).  A phase ends where the kernel has a wave_lds_fence(): every lane finishes it
// before any lane goes on.  Then the generic path's accumulate and fold thread programs over packed spectra.
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

// One launch of pspec1k_kernel: nunits units (rows, or with `split` segments) of the stream x; win: 1024 values or null; dst:
// 1024 f32 per unit; stores: writes per element of dst.
extern "C" void emu_pspec1k(const float2 *x, long step, long K, const float *win, int split, long nunits, float *dst, int *stores)
{
    const std::vector<float2> tw = make_tw(1024);
    static float2 v[64][16];
    static float w[64][16], seg[64][16], row[64][16];
    for (long u = 0; u < nunits; ++u) {
        long g0, cnt;
        pspec_unit(u, K, split != 0, g0, cnt);
        if (win)
            for (int lane = 0; lane < 64; ++lane) pspec1k_load_window(w[lane], win, lane);
        for (long i = 0; i < cnt; ++i) {
            for (int lane = 0; lane < 64; ++lane) {
                pspec1k_load(v[lane], x + (g0 + i) * step, lane);
                if (win) pspec1k_window(v[lane], w[lane]);
            }
            wave_fft(v, tw);
            const PspecStep s = pspec_step(i, cnt);
            for (int lane = 0; lane < 64; ++lane) {
                pspec1k_accum(v[lane], seg[lane], s.seg_first);
                if (s.seg_last) pspec1k_fold(seg[lane], row[lane], s.row_first);
            }
        }
        for (int lane = 0; lane < 64; ++lane) pspec1k_store(row[lane], Counted{dst + u * 1024, stores + u * 1024}, lane);
    }
}

// pspec_accum_kernel's threads over every segment of nrows rows of K packed spectra of N bins (part: N f32 per segment), then
// pspec_fold_kernel's threads (out: N f32 per row); stores_part / stores_out: writes per element
extern "C" void emu_pspec_generic(const float2 *spec, long N, long K, long nrows, float *part, float *out, int *stores_part, int *stores_out)
{
    const long S = pspec_nseg(K);
    for (long q = 0; q < nrows * S; ++q)
        for (long k = 0; k < N; ++k) {
            long g, cnt;
            pspec_segment(q, K, S, g, cnt);
            part[q * N + k] = pspec_accum_thread(spec + g * N, N, cnt, k);
            ++stores_part[q * N + k];
        }
    for (long r = 0; r < nrows; ++r)
        for (long k = 0; k < N; ++k) {
            out[r * N + k] = pspec_fold_thread(part + r * S * N, N, S, k);
            ++stores_out[r * N + k];
        }
}
