// pspec_real_api.hip -- C ABI of the real-input integrated power spectrum (include/redio.h, redio_pspec_real_*): |X[k]|^2 of kiss_fftr
// (tools/kiss_fftr.c, the bits of redio_fftr_*) summed over K consecutive transforms of N = nfft REAL samples that start every `step`
// samples, optionally windowed; B = N / 2 + 1 bins per row.  The integration is the stated design of DESIGN.md 5.3c (pspec_core.h:
// segments of REDIO_PSPEC_SEG transforms, a left fold inside each, a left fold over them); the contract is DESIGN.md 5.3d.
// Algorithmic bytes per real sample: 4 N / step read + 4 B / (K step) written.
//   N = 2048     one kernel: the spectra stay in the wave's registers (pspec_real_kernels.hip); one more fold pass when a wave takes a
//                segment instead of a whole row
//   other N      [row gather with window ->] the plan's own forward redio_fftr -> accumulate -> fold, through plan-owned scratch, in
//                chunks of whole segments with at most 64 MiB of spectra
#include "../../include/redio.h"
#include "redio_internal.h"
#include "pspec_real_core.h"
#include <new>

using namespace redio;

struct redio_pspec_real {
    int device, nfft;
    size_t B;              // nfft / 2 + 1 bins
    size_t K, step, S;     // S = ceil(K / 16) segments per row
    bool fused;            // N = 2048: one kernel
    bool packs;            // generic path: rows are always gathered (window or step != N); otherwise only a 4-byte aligned stream is
    int split;             // 0 auto, 1 one wave / thread group per row, 2 one per segment
    redio_fftr *fftr;      // forward, size N: twiddles, super twiddles, the generic transform
    float *d_win;          // N window values, or null
    size_t chunk_segs;     // generic path: segments per pass through the scratch
    void *d_rows;          // generic path: rows_cap gathered rows of N f32
    size_t rows_cap;
    void *d_spec;          // generic path: spec_cap spectra of B cf32
    size_t spec_cap;
    size_t fftr_cap;       // rows per call the plan's redio_fftr has been reserved for
    void *d_part;          // segment partials: part_cap f32
    size_t part_cap;
};

extern "C" int redio_pspec_real_create(redio_pspec_real **h, int nfft, size_t integrate, size_t step, const float *window_host)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (nfft < 2 || (nfft & 1) || integrate == 0 || step == 0) return REDIO_ERR_ARG;
    redio_fftr *fftr = nullptr;
    if (int rc = redio_fftr_create(&fftr, nfft, 0)) return rc; // its own refusals: the size ceiling, no device
    redio_pspec_real *p = new (std::nothrow) redio_pspec_real();
    if (!p) { redio_fftr_destroy(fftr); return REDIO_ERR_NOMEM; }
    p->device = 0; p->nfft = nfft; p->B = (size_t)nfft / 2 + 1; p->K = integrate; p->step = step; p->S = (size_t)pspec_nseg((long)integrate);
    p->fused = nfft == 2 * FFTR1K_M;
    p->packs = window_host != nullptr || step != (size_t)nfft;
    p->split = 0; p->fftr = fftr; p->d_win = nullptr;
    p->d_rows = p->d_spec = p->d_part = nullptr; p->rows_cap = p->spec_cap = p->part_cap = p->fftr_cap = 0;
    // at most 64 MiB of spectra per chunk (the overlap-save operators' work-buffer size), a whole number of segments, at least one
    p->chunk_segs = ((size_t)64 << 20) / (p->B * sizeof(float2) * PSPEC_SEG);
    if (p->chunk_segs < 1) p->chunk_segs = 1;
    int rc = hip_rc(hipGetDevice(&p->device));
    if (rc == REDIO_OK && window_host) {
        rc = hip_rc(hipMalloc((void **)&p->d_win, (size_t)nfft * sizeof(float)));
        if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(p->d_win, window_host, (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
    }
    if (rc != REDIO_OK) {
        redio_pspec_real_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_pspec_real_destroy(redio_pspec_real *h)
{
    if (!h) return REDIO_OK;
    redio_fftr_destroy(h->fftr);
    if (h->d_win) hipFree(h->d_win);
    redio_free(h->d_rows); redio_free(h->d_spec); redio_free(h->d_part);
    delete h;
    return REDIO_OK;
}

void redio_pspec_real_shape(const redio_pspec_real *h, int *nfft, size_t *K, size_t *step, int *device) { *nfft = h->nfft; *K = h->K; *step = h->step; *device = h->device; }

extern "C" size_t redio_pspec_real_nrows(const redio_pspec_real *h, size_t n_in)
{
    if (!h) return 0;
    const size_t W = (h->K - 1) * h->step + (size_t)h->nfft, H = h->K * h->step;
    return n_in < W ? 0 : (n_in - W) / H + 1;
}

extern "C" size_t redio_pspec_real_nbins(const redio_pspec_real *h) { return h ? h->B : 0; }

extern "C" int redio_pspec_real_is_fused(const redio_pspec_real *h) { return h && h->fused ? 1 : 0; }

extern "C" int redio_pspec_real_set_split(redio_pspec_real *h, int mode)
{
    if (!h || mode < 0 || mode > 2) return REDIO_ERR_ARG;
    h->split = mode;
    return REDIO_OK;
}

// whether a call of nrows rows leaves segment partials and runs the fold pass.  The fused kernel chooses; the generic accumulate
// pass always works by segments, so it folds whenever a row has more than one.
static bool splits(const redio_pspec_real *h, size_t nrows, bool fused_kernel)
{
    if (h->S < 2) return false;
    if (!fused_kernel) return true;
    return h->split == 2 || (h->split == 0 && nrows < (size_t)PSPEC_REAL_SPLIT_ROWS);
}

// transforms per pass of the generic path
static size_t pass_rows(const redio_pspec_real *h, size_t nrows)
{
    const size_t all = nrows * h->K, most = h->chunk_segs * PSPEC_SEG;
    return all < most ? all : most;
}

static int reserve_rows(redio_pspec_real *h, size_t nrows, bool fused_kernel, bool transforms)
{
    if (nrows == 0) return REDIO_OK;
    REDIO_TRY(hipSetDevice(h->device));
    if (splits(h, nrows, fused_kernel))
        if (int rc = scratch_grow(&h->d_part, &h->part_cap, nrows * h->S * h->B, sizeof(float))) return rc;
    if (!transforms) return REDIO_OK;
    const size_t ntr = pass_rows(h, nrows);
    if (ntr > h->fftr_cap) {
        if (int rc = redio_fftr_reserve(h->fftr, ntr)) return rc;
        h->fftr_cap = ntr;
    }
    // the row scratch on every plan: a stream that is only 4-byte aligned is gathered even without a window at step == N
    if (int rc = scratch_grow(&h->d_rows, &h->rows_cap, ntr * (size_t)h->nfft, sizeof(float))) return rc;
    return scratch_grow(&h->d_spec, &h->spec_cap, ntr * h->B, sizeof(float2));
}

extern "C" int redio_pspec_real_reserve(redio_pspec_real *h, size_t n_in)
{
    if (!h) return REDIO_ERR_ARG;
    // the partials are sized as the segment mode and redio_pspec_real_enqueue_spectra need them, whatever set_split says now
    return reserve_rows(h, redio_pspec_real_nrows(h, n_in), false, !h->fused);
}

// the accumulate half over packed spectra of B bins: segments [q0, q1) of the call, whose transform g_base is spec's first row
static int accumulate(redio_pspec_real *h, const float2 *spec, size_t q0, size_t q1, long g_base, float *out, bool split, hipStream_t st)
{
    return hip_rc(launch_pspec_accum(spec, split ? (float *)h->d_part : out, (long)q0, (long)(q1 - q0), (long)h->B, (long)h->K, g_base, st));
}

extern "C" int redio_pspec_real_enqueue(redio_pspec_real *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t nrows = redio_pspec_real_nrows(h, n_in);
    if (nrows == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 3) || ((uintptr_t)d_out & 3)) return REDIO_ERR_ARG;
    const size_t N = (size_t)h->nfft, B = h->B;
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + nrows * B * sizeof(float) && o < a + n_in * sizeof(float)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const float *x = (const float *)d_in;
    float *out = (float *)d_out;
    const bool split = splits(h, nrows, h->fused);
    const size_t pass = pass_rows(h, nrows);
    const bool short_part = split && nrows * h->S * B > h->part_cap;
    const bool short_rows = !h->fused && (pass * N > h->rows_cap || pass * B > h->spec_cap || pass > h->fftr_cap);
    if (short_part || short_rows) { // grown on first use unless redio_pspec_real_reserve() sized it; never during graph capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = reserve_rows(h, nrows, h->fused, !h->fused)) return rc;
    }
    if (h->fused) {
        REDIO_TRY(launch_pspecr2k(x, (long)h->step, (long)h->K, h->d_win, redio_fftr_twiddles_dev(h->fftr), redio_fftr_super_dev(h->fftr),
                                  split ? (float *)h->d_part : out, (long)(split ? nrows * h->S : nrows), split, st));
    } else {
        const size_t nseg = nrows * h->S;
        float *rows = (float *)h->d_rows;
        float2 *spec = (float2 *)h->d_spec;
        const bool gathers = h->packs || ((uintptr_t)d_in & 7); // the transform reads its rows as cf32: 8-byte aligned
        for (size_t q0 = 0; q0 < nseg; q0 += h->chunk_segs) {
            const size_t q1 = nseg - q0 < h->chunk_segs ? nseg : q0 + h->chunk_segs;
            long g0, g1, cnt;
            pspec_segment((long)q0, (long)h->K, (long)h->S, g0, cnt);
            pspec_segment((long)q1 - 1, (long)h->K, (long)h->S, g1, cnt);
            const size_t ntr = (size_t)(g1 + cnt - g0);
            if (gathers) {
                REDIO_TRY(launch_pspec_real_rows(x + (size_t)g0 * h->step, h->d_win, rows, (long)ntr, (long)N, (long)h->step, st));
                if (int rc = redio_fftr_enqueue(h->fftr, rows, spec, ntr, stream)) return rc;
            } else { // the transform reads the caller's buffer
                if (int rc = redio_fftr_enqueue_strided(h->fftr, x + (size_t)g0 * N, spec, ntr, (long)N, (long)B, stream)) return rc;
            }
            if (int rc = accumulate(h, spec, q0, q1, g0, out, split, st)) return rc;
        }
    }
    if (split) REDIO_TRY(launch_pspec_fold((const float *)h->d_part, out, (long)nrows, (long)B, (long)h->S, st));
    return REDIO_OK;
}

extern "C" int redio_pspec_real_enqueue_spectra(redio_pspec_real *h, const void *d_spectra, size_t nbatch, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t nrows = nbatch / h->K;
    if (nrows == 0) return REDIO_OK;
    if (!d_spectra || !d_out || ((uintptr_t)d_spectra & 7) || ((uintptr_t)d_out & 3)) return REDIO_ERR_ARG;
    const size_t B = h->B;
    const char *a = (const char *)d_spectra, *o = (const char *)d_out;
    if (a < o + nrows * B * sizeof(float) && o < a + nbatch * B * sizeof(float2)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const bool split = splits(h, nrows, false);
    if (split && nrows * h->S * B > h->part_cap) {
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = reserve_rows(h, nrows, false, false)) return rc;
    }
    if (int rc = accumulate(h, (const float2 *)d_spectra, 0, nrows * h->S, 0, (float *)d_out, split, st)) return rc;
    if (split) REDIO_TRY(launch_pspec_fold((const float *)h->d_part, (float *)d_out, (long)nrows, (long)B, (long)h->S, st));
    return REDIO_OK;
}
