// The front of the oversampled channelizer's workgroup kernel (libredio_amd/csrc/pfb_os_p2.hip, pfb_os_p2_kernel; route 2) run on the
// CPU: every thread of every workgroup, with the launcher's stream geometry and the functions of pfb_os_p2_core.h -- the prologue and
// the iteration loads (clamped, every index fenced against the samples the call may read), the two register sets swapping roles, the
// two windows and their rotation, the fold (both roundings), the store into the image, and the row loop of the output stores.  What
// lies between the image and the stores is fft_p2.h's transform, which pfb_p2_kernel shares and the GPU tests cover.
#include "../../libredio_amd/csrc/pfb_os_p2_core.h"
#include <vector>

using namespace redio;

namespace {
constexpr int MAXC = 4, MAXP = 16, MAXTR = 16;
struct Thread {
    float gt[MAXC][MAXP];
    float2 hist[MAXC][2][MAXP - 1], ra[MAXC][MAXTR], rb[MAXC][MAXTR];
};

// error codes
constexpr long E_SHAPE = -1, E_FENCE = -2, E_IMAGE = -3, E_LOADS = -4, E_SPACE = -5;

template <int LOG2M>
long emu(const float2 *x, long n_valid, const float *h, int P, bool pair, bool fused, long rows, int fpar, long cus, long rps, float2 *img, int *stores,
         long *geom, long max_groups)
{
    constexpr int M = 1 << LOG2M;
    // pfb_os_p2_kernel's shape constants
    const int NP = pair ? (M <= 512 ? 1 : M / 512) : (M <= 256 ? 1 : M / 256);
    const int CPT = pair ? 2 * NP : NP, MT = M / CPT, G = 256 / MT, TR = 16 / CPT, HR = TR / 2;
    if (G != pfbos_p2_streams_per_group(M) || TR != pfbos_p2_rows_per_iter(M) || G * TR * M != 4096 || TR % 2 || (pair && M < 512)) return E_SHAPE;
    if (rps <= 0) rps = pfbos_p2_rows_per_stream(rows, cus, M);
    if (rps % TR) return E_SHAPE; // a stream starts on an even row of the call
    const long grid = pfbos_p2_groups(rows, rps, M);
    if (grid > max_groups) return E_SPACE;
    geom[0] = rps; geom[1] = pfbos_p2_streams(rows, rps); geom[2] = grid;
    auto chan = [&](int m, int c) { return pair ? 2 * m + (c & 1) + 512 * (c >> 1) : m + 256 * c; };
    long err = 0;
    std::vector<Thread> th(256);
    for (long b = 0; b < grid; ++b) {
        const long s0 = b * G;
        const long iters = pfbos_p2_group_iters(b, rps, rows, M);
        // requests per (half-row, channel) of each stream, by the half-row ASKED for (before the clamp), counted from the stream's first
        const long nq = 2 * (P - 1) + TR * (iters + 1);
        std::vector<int> asked((size_t)G * nq * M, 0);
        // one row load of thread (m, g): ld_half of the kernel
        auto ld_half = [&](int m, int g, long t0, long q, float2 *dst, int step) {
            const long qc = pfbos_p2_half(q, rows, P);
            for (int u = 0; u < NP; ++u)
                for (int w = 0; w < (pair ? 2 : 1); ++w) {
                    const int c = pair ? 2 * u + w : u;
                    const long i = pfbos_p2_in_index(qc, chan(m, c), M);
                    if (i < 0 || i >= n_valid) { err = E_FENCE; return; }
                    if (q - t0 < 0 || q - t0 >= nq) { err = E_LOADS; return; }
                    ++asked[((size_t)g * nq + (q - t0)) * M + chan(m, c)];
                    dst[c * step] = x[i];
                }
        };
        for (int tid = 0; tid < 256; ++tid) { // the prologue
            Thread &t = th[tid];
            const int m = tid % MT, g = tid / MT;
            const long t0 = pfbos_p2_stream_begin(s0 + g, rps);
            for (int c = 0; c < CPT; ++c)
                for (int p = 0; p < P; ++p) t.gt[c][p] = h[M * p + chan(m, c)];
            for (int p = 0; p < P - 1; ++p)
                for (int par = 0; par < 2; ++par) ld_half(m, g, t0, pfbos_p2_hist_half(t0, par, p), &t.hist[0][par][p], 2 * (MAXP - 1));
            for (int ti = 0; ti < TR; ++ti) ld_half(m, g, t0, pfbos_p2_enter(t0 + ti, P), &t.ra[0][ti], MAXTR);
        }
        if (err) return err;
        for (long it = 0; it < iters; ++it) {
            std::vector<float2> image(4096);
            std::vector<int> written(4096, 0);
            for (int tid = 0; tid < 256; ++tid) {
                Thread &t = th[tid];
                const int m = tid % MT, g = tid / MT;
                const long t0 = pfbos_p2_stream_begin(s0 + g, rps), tb = t0 + (long)TR * it;
                float2(&cur)[MAXC][MAXTR] = (it & 1) ? t.rb : t.ra; // the two register sets swap roles
                float2(&nx)[MAXC][MAXTR] = (it & 1) ? t.ra : t.rb;
                for (int ti = 0; ti < TR; ++ti) ld_half(m, g, t0, pfbos_p2_enter(tb + TR + ti, P), &nx[0][ti], MAXTR);
                for (int c = 0; c < CPT; ++c) {
                    const int lp[2] = {(TR * g) * M + pfbos_p2_image_pos<LOG2M>(chan(m, c), 0, fpar), (TR * g) * M + pfbos_p2_image_pos<LOG2M>(chan(m, c), 1, fpar)};
                    for (int ti = 0; ti < TR; ++ti) {
                        const int par = ti & 1;
                        float2 acc = make_float2(0.f, 0.f);
                        for (int p = 0; p < P; ++p) {
                            const int k = pfbos_p2_win(ti, p);
                            const float2 v = k < P - 1 ? t.hist[c][par][k] : cur[c][pfbos_p2_cur_slot(par, k, P)];
                            acc = fused ? mac<true>(v, t.gt[c][p], acc) : mac<false>(v, t.gt[c][p], acc);
                        }
                        const int e = lp[par] + ti * M;
                        if (e < 0 || e >= 4096) return E_IMAGE;
                        image[e] = acc; ++written[e];
                    }
                    for (int par = 0; par < 2; ++par) {
                        float2 hn[MAXP - 1];
                        for (int p = 0; p < P - 1; ++p) hn[p] = p + HR < P - 1 ? t.hist[c][par][p + HR] : cur[c][pfbos_p2_cur_slot(par, p + HR, P)];
                        for (int p = 0; p < P - 1; ++p) t.hist[c][par][p] = hn[p];
                    }
                }
            }
            if (err) return err;
            for (int e = 0; e < 4096; ++e)
                if (written[e] != 1) return E_IMAGE; // each image position exactly once per iteration
            // the row loop of the output stores (the transform left out): the image's rows to img, in image order
            for (int tid = 0; tid < 256; ++tid)
                for (int e = 2 * tid; e < 4096; e += 512) {
                    const int xf = e / M, n = e % M, gg = xf / TR, ti = xf % TR;
                    const long row = pfbos_p2_stream_begin(s0 + gg, rps) + (long)TR * it + ti;
                    if (row < pfbos_p2_stream_end(s0 + gg, rps, rows)) {
                        img[row * M + n] = image[e]; img[row * M + n + 1] = image[e + 1];
                        ++stores[row * M + n]; ++stores[row * M + n + 1];
                    }
                }
        }
        for (int v : asked)
            if (v != 1) return E_LOADS; // every s_q[m] of a stream is asked for exactly once
    }
    return grid;
}
} // namespace

// One launch on x[0, n_valid) (the samples the call may read: (rows - 1) M / 2 + M P).  pair: the load form (512 and 1024 channels
// only); F: first_row; rps: rows per stream, 0 for the launcher's own choice on a device of `cus` CUs.  img: rows x M, row r of the
// image behind the branch filters in IMAGE order (leaf positions); stores: writes per element of the output; geom: {rps, streams,
// workgroups}.  Returns the workgroup count, or a negative code: -1 shape constants disagree with pfb_os_p2_core.h, -2 a load outside
// [0, n_valid), -3 an image position written twice or never, -4 a half-row asked for twice or never, -5 max_groups too small.
extern "C" long emu_pfb_os_p2(const float2 *x, long n_valid, const float *h, int M, int P, int pair, int fused, long rows, unsigned long long F, long cus,
                              long rps, float2 *img, int *stores, long *geom, long max_groups)
{
    if (P < 2 || P > MAXP || rows <= 0) return E_SHAPE;
    const int fpar = (int)(F & 1);
    switch (M) {
    case 32: return emu<5>(x, n_valid, h, P, pair != 0, fused != 0, rows, fpar, cus, rps, img, stores, geom, max_groups);
    case 128: return emu<7>(x, n_valid, h, P, pair != 0, fused != 0, rows, fpar, cus, rps, img, stores, geom, max_groups);
    case 256: return emu<8>(x, n_valid, h, P, pair != 0, fused != 0, rows, fpar, cus, rps, img, stores, geom, max_groups);
    case 512: return emu<9>(x, n_valid, h, P, pair != 0, fused != 0, rows, fpar, cus, rps, img, stores, geom, max_groups);
    case 1024: return emu<10>(x, n_valid, h, P, pair != 0, fused != 0, rows, fpar, cus, rps, img, stores, geom, max_groups);
    }
    return E_SHAPE;
}

// the launcher's own numbers, for the tests' restatement of them
extern "C" long emu_pfb_os_p2_rows_per_stream(long rows, long cus, int M) { return pfbos_p2_rows_per_stream(rows, cus, M); }
extern "C" int emu_pfb_os_p2_streams_per_group(int M) { return pfbos_p2_streams_per_group(M); }
extern "C" int emu_pfb_os_p2_rows_per_iter(int M) { return pfbos_p2_rows_per_iter(M); }
extern "C" long emu_pfb_os_p2_streams(long rows, long rps) { return pfbos_p2_streams(rows, rps); }
extern "C" long emu_pfb_os_p2_groups(long rows, long rps, int M) { return pfbos_p2_groups(rows, rps, M); }

#ifdef EMU_PFB_OS_P2_MAIN
// stand-alone run (host sanitizers): a small launch of every shape and load form on a ramp, every check of emu() armed
#include <stdio.h>
int main()
{
    const int Ms[5] = {32, 128, 256, 512, 1024}, Ps[3] = {4, 8, 16};
    for (int M : Ms)
        for (int P : Ps)
            for (int pair = 0; pair < (M >= 512 ? 2 : 1); ++pair)
                for (long rows : {1L, 17L, 65L, 133L}) {
                    const long n = (rows - 1) * (M / 2) + (long)M * P;
                    std::vector<float2> x((size_t)n), img((size_t)rows * M);
                    std::vector<float> h((size_t)M * P);
                    std::vector<int> stores((size_t)rows * M, 0);
                    for (long i = 0; i < n; ++i) x[i] = make_float2((float)(i % 97) - 48.f, (float)(i % 89) * 0.25f);
                    for (long i = 0; i < (long)M * P; ++i) h[i] = (float)(i % 13) * 0.125f - 0.5f;
                    long geom[3];
                    const long g = emu_pfb_os_p2(x.data(), n, h.data(), M, P, pair, 1, rows, 1, 1, 0, img.data(), stores.data(), geom, 1 << 20);
                    bool ok = g > 0;
                    for (int s : stores) ok = ok && s == 1;
                    if (!ok) { printf("FAIL M=%d P=%d pair=%d rows=%ld rc=%ld\n", M, P, pair, rows, g); return 1; }
                }
    printf("emu_pfb_os_p2 ok\n");
    return 0;
}
#endif
