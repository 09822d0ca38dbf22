// pspec_api.hip -- C ABI of the integrated power spectrum (include/redio.h, redio_pspec_*): |X[k]|^2 of the kissfft::fft block
// (src/kissfft/src/kissfft.rs:18-31) summed over K consecutive transforms of N = nfft samples that start every `step` samples,
// optionally windowed (the periodogram; with a window and step < N, Welch's method).  The integration is new: the reference has no
// such block.  Summation order (pspec_core.h): segments of REDIO_PSPEC_SEG transforms, a left fold inside each, a left fold over them.
// Algorithmic bytes per input sample: 8 N / step read + 4 / K written.
//   N = 1024     one kernel: the spectra stay in the wave's registers (pspec_kernels.hip); one more fold pass when a wave takes a
//                segment instead of a whole row
//   other N      [row gather with window ->] the plan's own redio_fft -> accumulate -> fold, through plan-owned scratch, in chunks
//                of whole segments
// redio_pspec_enqueue_u8 is the same plan fed with the receiver's interleaved u8 I/Q bytes (rtlsdr.rs:159-162), bit for bit
// redio_data_to_samples + redio_pspec_enqueue: N = 1024 is the fused kernel with the conversion at the load (2 N / step bytes read
// per sample); at 2048 and 4096 the plan's one-wave transform has a sibling that converts and windows at its own load
// (fft_kernels.hip, launch_fft_u8); every other N converts inside the row gather -- there is never a whole-message cf32 buffer.
#include "../../include/redio.h"
#include "redio_internal.h"
#include "pspec_core.h"
#include <new>

using namespace redio;

static_assert(PSPEC_SEG == REDIO_PSPEC_SEG, "the header's constant is the kernels'");


struct redio_pspec {
    int device, nfft;
    size_t K, step, S;     // S = ceil(K / 16) segments per row
    bool fused;            // N = 1024: one kernel
    bool packs;            // generic path: rows are gathered (window or step != N) before the transform, which then runs in place
    bool fft_stages;       // the plan's transform stages through a buffer of its own at this size (redio_fft_reserve)
    bool fft_stages_packed; // the same for a packed chunk transformed in place: what a u8 call runs on every plan (== fft_stages when packs)
    size_t packed_cap;     // transforms per pass for which the in-place transform's staging has been reserved
    bool fft_u8;           // the transform has a sibling that converts (and windows) bytes at its own load (2048, 4096): a u8 call needs no gather
    int split;             // 0 auto, 1 one wave / thread group per row, 2 one per segment
    redio_fft *fft;
    float *d_win;          // N window values, or null
    size_t chunk_segs;     // generic path: segments per pass through the scratch
    void *d_rows;          // generic path: rows_cap rows of N cf32
    size_t rows_cap;
    void *d_part;          // segment partials: part_cap f32
    size_t part_cap;
};

extern "C" int redio_pspec_create(redio_pspec **h, int nfft, size_t integrate, size_t step, const float *window_host)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (nfft < 1 || integrate == 0 || step == 0) return REDIO_ERR_ARG;
    redio_fft *fft = nullptr;
    if (int rc = redio_fft_create(&fft, nfft, 0)) return rc; // its own refusals: the size ceiling, no device
    redio_pspec *p = new (std::nothrow) redio_pspec();
    if (!p) { redio_fft_destroy(fft); return REDIO_ERR_NOMEM; }
    p->device = 0; p->nfft = nfft; p->K = integrate; p->step = step; p->S = (size_t)pspec_nseg((long)integrate);
    p->fused = nfft == 1024;
    p->packs = window_host != nullptr || step != (size_t)nfft;
    p->split = 0; p->fft = fft; p->d_win = nullptr; p->d_rows = p->d_part = nullptr; p->rows_cap = p->part_cap = 0;
    p->fft_stages = redio_fft_stages(fft, p->packs); // a packed chunk is transformed in place
    p->fft_u8 = fft_u8_supported(*redio_fft_plan_dev(fft));
    p->fft_stages_packed = !p->fft_u8 && redio_fft_stages(fft, true);
    p->packed_cap = 0;
    // at most 64 MiB of cf32 rows per chunk (the overlap-save operators' work-buffer size), a whole number of segments, at least one
    p->chunk_segs = ((size_t)64 << 20) / ((size_t)nfft * sizeof(float2) * PSPEC_SEG);
    if (p->chunk_segs < 1) p->chunk_segs = 1;
    int rc = hip_rc(hipGetDevice(&p->device));
    if (rc == REDIO_OK && window_host) {
        rc = hip_rc(hipMalloc((void **)&p->d_win, (size_t)nfft * sizeof(float)));
        if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(p->d_win, window_host, (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
    }
    if (rc != REDIO_OK) {
        redio_pspec_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_pspec_destroy(redio_pspec *h)
{
    if (!h) return REDIO_OK;
    redio_fft_destroy(h->fft);
    if (h->d_win) hipFree(h->d_win);
    redio_free(h->d_rows); redio_free(h->d_part);
    delete h;
    return REDIO_OK;
}

void redio_pspec_shape(const redio_pspec *h, int *nfft, size_t *K, size_t *step, int *device) { *nfft = h->nfft; *K = h->K; *step = h->step; *device = h->device; }

extern "C" size_t redio_pspec_nrows(const redio_pspec *h, size_t n_in)
{
    if (!h) return 0;
    const size_t W = (h->K - 1) * h->step + (size_t)h->nfft, H = h->K * h->step;
    return n_in < W ? 0 : (n_in - W) / H + 1;
}

extern "C" int redio_pspec_is_fused(const redio_pspec *h) { return h && h->fused ? 1 : 0; }

extern "C" int redio_pspec_set_split(redio_pspec *h, int mode)
{
    if (!h || mode < 0 || mode > 2) return REDIO_ERR_ARG;
    h->split = mode;
    return REDIO_OK;
}

// whether a call of nrows rows leaves segment partials and runs the fold pass.  The fused kernel chooses; the generic accumulate
// pass always works by segments, so it folds whenever a row has more than one.
static bool splits(const redio_pspec *h, size_t nrows, bool fused_kernel)
{
    if (h->S < 2) return false;
    if (!fused_kernel) return true;
    return h->split == 2 || (h->split == 0 && nrows < (size_t)PSPEC_SPLIT_ROWS);
}

static size_t rows_needed(const redio_pspec *h, size_t nrows)
{
    const size_t all = nrows * h->K, most = h->chunk_segs * PSPEC_SEG;
    return all < most ? all : most;
}

// packed: sized for a u8 call, which gathers rows and transforms them in place on every plan
static int reserve_rows(redio_pspec *h, size_t nrows, bool fused_kernel, bool transforms, bool packed = false)
{
    if (nrows == 0) return REDIO_OK;
    REDIO_TRY(hipSetDevice(h->device));
    if (splits(h, nrows, fused_kernel))
        if (int rc = scratch_grow(&h->d_part, &h->part_cap, nrows * h->S * (size_t)h->nfft, sizeof(float))) return rc;
    if (!transforms) return REDIO_OK;
    const size_t ntr = rows_needed(h, nrows);
    if (packed ? h->fft_stages_packed : h->fft_stages) {
        if (int rc = redio_fft_reserve(h->fft, ntr)) return rc;
        if ((packed || h->packs) && ntr > h->packed_cap) h->packed_cap = ntr;
    }
    return scratch_grow(&h->d_rows, &h->rows_cap, ntr * (size_t)h->nfft, sizeof(float2));
}

extern "C" int redio_pspec_reserve(redio_pspec *h, size_t n_in)
{
    if (!h) return REDIO_ERR_ARG;
    // the partials are sized as the segment mode and redio_pspec_enqueue_spectra need them, whatever redio_pspec_set_split says now
    return reserve_rows(h, redio_pspec_nrows(h, n_in), false, !h->fused);
}

// the accumulate and fold half over packed spectra: segments [q0, q1) of the call, whose transform g_base is spec's first row
static int accumulate(redio_pspec *h, const float2 *spec, size_t q0, size_t q1, long g_base, float *out, bool split, hipStream_t st)
{
    return hip_rc(launch_pspec_accum(spec, split ? (float *)h->d_part : out, (long)q0, (long)(q1 - q0), h->nfft, (long)h->K, g_base, st));
}

extern "C" int redio_pspec_enqueue(redio_pspec *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t nrows = redio_pspec_nrows(h, n_in);
    if (nrows == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 3)) return REDIO_ERR_ARG;
    const size_t N = (size_t)h->nfft;
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + nrows * N * sizeof(float) && o < a + n_in * sizeof(float2)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const float2 *x = (const float2 *)d_in;
    float *out = (float *)d_out;
    const bool split = splits(h, nrows, h->fused);
    const bool short_part = split && nrows * h->S * N > h->part_cap;
    const bool short_rows = !h->fused && rows_needed(h, nrows) * N > h->rows_cap;
    if (short_part || short_rows) { // grown on first use unless redio_pspec_reserve() sized it; never during graph capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = reserve_rows(h, nrows, h->fused, !h->fused)) return rc;
    }
    if (h->fused) {
        REDIO_TRY(launch_pspec1k(x, (long)h->step, (long)h->K, h->d_win, redio_fft_twiddles_dev(h->fft), split ? (float *)h->d_part : out,
                              (long)(split ? nrows * h->S : nrows), split, st));
    } else {
        const size_t nseg = nrows * h->S;
        float2 *rows = (float2 *)h->d_rows;
        for (size_t q0 = 0; q0 < nseg; q0 += h->chunk_segs) {
            const size_t q1 = nseg - q0 < h->chunk_segs ? nseg : q0 + h->chunk_segs;
            long g0, g1, cnt;
            pspec_segment((long)q0, (long)h->K, (long)h->S, g0, cnt);
            pspec_segment((long)q1 - 1, (long)h->K, (long)h->S, g1, cnt);
            const size_t ntr = (size_t)(g1 + cnt - g0);
            if (h->packs) {
                REDIO_TRY(launch_pspec_rows(x + (size_t)g0 * h->step, h->d_win, rows, (long)ntr, (long)N, (long)h->step, st));
                if (int rc = redio_fft_enqueue(h->fft, rows, rows, ntr, stream)) return rc;
            } else {
                if (int rc = redio_fft_enqueue(h->fft, x + (size_t)g0 * N, rows, ntr, stream)) return rc;
            }
            if (int rc = accumulate(h, rows, q0, q1, g0, out, split, st)) return rc;
        }
    }
    if (split) REDIO_TRY(launch_pspec_fold((const float *)h->d_part, out, (long)nrows, (long)N, (long)h->S, st));
    return REDIO_OK;
}

extern "C" int redio_pspec_reserve_u8(redio_pspec *h, size_t nbytes)
{
    if (!h) return REDIO_ERR_ARG;
    return reserve_rows(h, redio_pspec_nrows(h, nbytes / 2), false, !h->fused, true);
}

extern "C" int redio_pspec_enqueue_u8(redio_pspec *h, const void *d_bytes, size_t nbytes, void *d_out, void *stream)
{
    if (!h || (nbytes & 1)) return REDIO_ERR_ARG;
    const size_t nrows = redio_pspec_nrows(h, nbytes / 2);
    if (nrows == 0) return REDIO_OK;
    if (!d_bytes || !d_out || ((uintptr_t)d_bytes & 1) || ((uintptr_t)d_out & 3)) return REDIO_ERR_ARG; // a sample-aligned pointer, as the cf32 entry asks for 8
    const size_t N = (size_t)h->nfft;
    const char *a = (const char *)d_bytes, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + nrows * N * sizeof(float) && o < a + nbytes) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const uint16_t *x = (const uint16_t *)d_bytes; // one word per sample
    float *out = (float *)d_out;
    const bool split = splits(h, nrows, h->fused);
    const size_t pass = rows_needed(h, nrows);
    const bool short_part = split && nrows * h->S * N > h->part_cap;
    const bool short_rows = !h->fused && (pass * N > h->rows_cap || (h->fft_stages_packed && pass > h->packed_cap));
    if (short_part || short_rows) { // grown on first use unless redio_pspec_reserve_u8() sized it; never during graph capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = reserve_rows(h, nrows, h->fused, !h->fused, true)) return rc;
    }
    if (h->fused) {
        REDIO_TRY(launch_pspec1k_u8(x, (long)h->step, (long)h->K, h->d_win, redio_fft_twiddles_dev(h->fft), split ? (float *)h->d_part : out,
                                 (long)(split ? nrows * h->S : nrows), split, st));
    } else {
        const size_t nseg = nrows * h->S;
        float2 *rows = (float2 *)h->d_rows;
        for (size_t q0 = 0; q0 < nseg; q0 += h->chunk_segs) {
            const size_t q1 = nseg - q0 < h->chunk_segs ? nseg : q0 + h->chunk_segs;
            long g0, g1, cnt;
            pspec_segment((long)q0, (long)h->K, (long)h->S, g0, cnt);
            pspec_segment((long)q1 - 1, (long)h->K, (long)h->S, g1, cnt);
            const size_t ntr = (size_t)(g1 + cnt - g0);
            if (h->fft_u8) { // the transform converts and windows at its own load: bytes in, spectra out
                REDIO_TRY(launch_fft_u8(*redio_fft_plan_dev(h->fft), x + (size_t)g0 * h->step, h->d_win, rows, (long)ntr, (long)h->step, st));
            } else {
                REDIO_TRY(launch_pspec_rows_u8(x + (size_t)g0 * h->step, h->d_win, rows, (long)ntr, (long)N, (long)h->step, st));
                if (int rc = redio_fft_enqueue(h->fft, rows, rows, ntr, stream)) return rc;
            }
            if (int rc = accumulate(h, rows, q0, q1, g0, out, split, st)) return rc;
        }
    }
    if (split) REDIO_TRY(launch_pspec_fold((const float *)h->d_part, out, (long)nrows, (long)N, (long)h->S, st));
    return REDIO_OK;
}

extern "C" int redio_pspec_enqueue_spectra(redio_pspec *h, const void *d_spectra, size_t nbatch, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t nrows = nbatch / h->K;
    if (nrows == 0) return REDIO_OK;
    if (!d_spectra || !d_out || ((uintptr_t)d_spectra & 7) || ((uintptr_t)d_out & 3)) return REDIO_ERR_ARG;
    const size_t N = (size_t)h->nfft;
    const char *a = (const char *)d_spectra, *o = (const char *)d_out;
    if (a < o + nrows * N * sizeof(float) && o < a + nbatch * N * sizeof(float2)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const bool split = splits(h, nrows, false);
    if (split && nrows * h->S * N > h->part_cap) {
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = reserve_rows(h, nrows, false, false)) return rc;
    }
    if (int rc = accumulate(h, (const float2 *)d_spectra, 0, nrows * h->S, 0, (float *)d_out, split, st)) return rc;
    if (split) REDIO_TRY(launch_pspec_fold((const float *)h->d_part, (float *)d_out, (long)nrows, (long)N, (long)h->S, st));
    return REDIO_OK;
}
