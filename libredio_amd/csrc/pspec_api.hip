// pspec_api.hip -- C ABI of the integrated power spectrum (include/redio.h, redio_pspec_* and redio_pspec_real_*): |X[k]|^2 summed over
// K consecutive transforms of N = nfft samples that start every `step` samples, optionally windowed (the periodogram; with a window
// and step < N, Welch's method).  The integration is new: the reference has no such block.  Summation order (pspec_core.h): segments
// of REDIO_PSPEC_SEG transforms, a left fold inside each, a left fold over them.  Three plans, one driver (enqueue<Entry> below):
//   redio_pspec        X = the kissfft::fft block (src/kissfft/src/kissfft.rs:18-31) of N cf32 samples, B = N bins per row; fused at
//                      N = 1024 (pspec_kernels.hip).  Algorithmic bytes per input sample: 8 N / step read + 4 / K written.
//   redio_pspec_real   X = kiss_fftr (tools/kiss_fftr.c, the bits of redio_fftr_*) of N REAL samples, B = N / 2 + 1 bins per row; fused
//                      at N = 2048 (pspec_real_kernels.hip).  Per real sample: 4 N / step read + 4 B / (K step) written.
//   redio_pfb_pspec    X = row t of the polyphase channelizer (redio_pfb_*, ngroups = 1) of M = nchan channels, B = M; a transform starts
//                      every M samples and reads P M of them; fused at 64 channels x 4 / 8 / 16 taps per branch (pfb_pspec_kernels.hip).
//                      With REDIO_PFB_PSPEC_BLOCK also at 32 / 128 / 256 / 512 / 1024 channels (pfb_pspec_p2.hip, `block` below).
//                      Per input sample: 8 (cf32) or 2 (u8 I/Q) bytes read + 4 / K written.  Contract: DESIGN.md 5.6b.
//   fused N      one kernel: the spectra stay in the wave's registers; one more fold pass when a wave takes a segment instead of a
//                whole row
//   other N      [row gather with window ->] the plan's own transform -> accumulate -> fold, through plan-owned scratch, in chunks of
//                whole segments with at most 64 MiB of spectra
// redio_pspec_enqueue_u8 is the complex plan fed with the receiver's interleaved u8 I/Q bytes (rtlsdr.rs:159-162), bit for bit
// redio_data_to_samples + redio_pspec_enqueue: N = 1024 is the fused kernel with the conversion at the load (2 N / step bytes read
// per sample); at 2048 and 4096 the plan's one-wave transform has a sibling that converts and windows at its own load
// (fft_kernels.hip, launch_fft_u8); every other N converts inside the row gather -- there is never a whole-message cf32 buffer.
#include "../../include/redio.h"
#include "redio_internal.h"
#include "pspec_real_core.h"
#include "pfb_pspec_p2_core.h"
#include <new>
#include <type_traits>

using namespace redio;

static_assert(PSPEC_SEG == REDIO_PSPEC_SEG, "the header's constant is the kernels'");

namespace {
// what both plans hold, and everything below that does not depend on the sample type works on
struct Pspec {
    int device, nfft;      // nfft: the samples one transform reads (redio_pfb_pspec: nchan * taps_per_branch)
    size_t B;              // bins per row: N, or N / 2 + 1 for the real plan
    size_t K, step, S;     // S = ceil(K / 16) segments per row
    bool fused;            // the plan's one-kernel size
    bool block;            // redio_pfb_pspec with REDIO_PFB_PSPEC_BLOCK on a pfb_p2 shape: the workgroup kernel (pfb_pspec_p2.hip), as
                           // `fused` for scratch purposes; redio_pfb_pspec_is_fused() stays the 64-channel wave kernel
    int split;             // 0 auto, 1 one wave / thread group per row, 2 one per segment
    long split_rows;       // auto: a wave per segment below this many rows (PSPEC_SPLIT_ROWS / PSPEC_REAL_SPLIT_ROWS)
    float *d_win;          // N window values, or null
    size_t chunk_segs;     // generic path: segments per pass through the scratch
    void *d_part;          // segment partials: part_cap f32
    size_t part_cap;
};

// a value-initialised Pspec in; on an error the caller's destroy frees what was made
int pspec_init(Pspec &c, int nfft, size_t bins, size_t K, size_t step, bool fused, long split_rows, const float *window_host)
{
    c.nfft = nfft; c.B = bins; c.K = K; c.step = step; c.S = (size_t)pspec_nseg((long)K);
    c.fused = fused; c.split_rows = split_rows;
    // at most 64 MiB of spectra per chunk (the overlap-save operators' work-buffer size), a whole number of segments, at least one
    c.chunk_segs = ((size_t)64 << 20) / (bins * sizeof(float2) * PSPEC_SEG);
    if (c.chunk_segs < 1) c.chunk_segs = 1;
    int rc = hip_rc(hipGetDevice(&c.device));
    if (rc == REDIO_OK && window_host) {
        rc = hip_rc(hipMalloc((void **)&c.d_win, (size_t)nfft * sizeof(float)));
        if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(c.d_win, window_host, (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
    }
    return rc;
}

void pspec_free(Pspec &c)
{
    if (c.d_win) hipFree(c.d_win);
    redio_free(c.d_part);
}

size_t nrows_of(const Pspec &c, size_t n_in)
{
    const size_t W = (c.K - 1) * c.step + (size_t)c.nfft, H = c.K * c.step;
    return n_in < W ? 0 : (n_in - W) / H + 1;
}

int set_split(Pspec &c, int mode)
{
    if (mode < 0 || mode > 2) return REDIO_ERR_ARG;
    c.split = mode;
    return REDIO_OK;
}

// whether a call of nrows rows leaves segment partials and runs the fold pass.  The fused kernel chooses; the generic accumulate
// pass always works by segments, so it folds whenever a row has more than one.
bool splits(const Pspec &c, size_t nrows, bool fused_kernel)
{
    if (c.S < 2) return false;
    if (!fused_kernel) return true;
    return c.split == 2 || (c.split == 0 && nrows < (size_t)c.split_rows);
}

// transforms per pass of the generic path
size_t pass_rows(const Pspec &c, size_t nrows)
{
    const size_t all = nrows * c.K, most = c.chunk_segs * PSPEC_SEG;
    return all < most ? all : most;
}

int grow_part(Pspec &c, size_t nrows) { return scratch_grow(&c.d_part, &c.part_cap, nrows * c.S * c.B, sizeof(float)); }

// the accumulate half over packed spectra of B bins: segments [q0, q1) of the call, whose transform g_base is spec's first row
int accumulate(const Pspec &c, const float2 *spec, size_t q0, size_t q1, long g_base, float *out, bool split, hipStream_t st)
{
    return hip_rc(launch_pspec_accum(spec, split ? (float *)c.d_part : out, (long)q0, (long)(q1 - q0), (long)c.B, (long)c.K, g_base, st));
}

// The one driver.  An Entry says what its input is:
//   align, in_bytes(n_in)   the input pointer's alignment mask and the bytes a call of n_in samples reads (the overlap check)
//   transforms              false for spectra in: never the fused kernel, no pass scratch, one pass over the caller's buffer
//   short_rows(pass)        whether its pass scratch is short for `pass` transforms;  reserve(pass) sizes it
//   launch_fused(...)       its one-kernel launch
//   spectra(...)            produces the spectra of transforms [g0, g0 + ntr) of the call and says where they are
template <typename E>
int enqueue(Pspec &c, const E &e, const void *d_in, size_t n_in, size_t nrows, void *d_out, void *stream)
{
    if (nrows == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & E::align) || ((uintptr_t)d_out & 3)) return REDIO_ERR_ARG;
    const size_t B = c.B;
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + nrows * B * sizeof(float) && o < a + e.in_bytes(n_in)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(c.device));
    hipStream_t st = (hipStream_t)stream;
    float *out = (float *)d_out;
    const bool fused = E::transforms && (c.fused || c.block);
    const bool split = splits(c, nrows, fused);
    const size_t pass = pass_rows(c, nrows);
    const bool short_part = split && nrows * c.S * B > c.part_cap;
    if (short_part || (!fused && e.short_rows(pass))) { // grown on first use unless the entry's reserve sized it; never during graph capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (split)
            if (int rc = grow_part(c, nrows)) return rc;
        if (!fused)
            if (int rc = e.reserve(pass)) return rc;
    }
    if (fused) {
        REDIO_TRY(e.launch_fused(d_in, split ? (float *)c.d_part : out, (long)(split ? nrows * c.S : nrows), split, st));
    } else {
        const size_t nseg = nrows * c.S, chunk = E::transforms ? c.chunk_segs : nseg;
        for (size_t q0 = 0; q0 < nseg; q0 += chunk) {
            const size_t q1 = nseg - q0 < chunk ? nseg : q0 + chunk;
            long g0, g1, cnt;
            pspec_segment((long)q0, (long)c.K, (long)c.S, g0, cnt);
            pspec_segment((long)q1 - 1, (long)c.K, (long)c.S, g1, cnt);
            const float2 *spec = nullptr;
            if (int rc = e.spectra(d_in, (size_t)g0, (size_t)(g1 + cnt - g0), stream, spec)) return rc;
            if (int rc = accumulate(c, spec, q0, q1, g0, out, split, st)) return rc;
        }
    }
    if (split) REDIO_TRY(launch_pspec_fold((const float *)c.d_part, out, (long)nrows, (long)B, (long)c.S, st));
    return REDIO_OK;
}

// the entry's *_reserve for a message of nrows rows: the partials as the segment mode and *_enqueue_spectra need them, whatever
// *_set_split says now, and the entry's pass scratch unless the plan is fused
template <typename E>
int reserve(Pspec &c, const E &e, size_t nrows)
{
    if (nrows == 0) return REDIO_OK;
    REDIO_TRY(hipSetDevice(c.device));
    if (splits(c, nrows, false))
        if (int rc = grow_part(c, nrows)) return rc;
    return c.fused || c.block ? REDIO_OK : e.reserve(pass_rows(c, nrows));
}

// packed, already transformed rows of B bins in (redio_pspec_enqueue_spectra, redio_pspec_real_enqueue_spectra): n_in counts spectra
struct Spectra {
    const Pspec &c;
    static constexpr bool transforms = false;
    static constexpr uintptr_t align = 7;
    size_t in_bytes(size_t nbatch) const { return nbatch * c.B * sizeof(float2); }
    bool short_rows(size_t) const { return false; }
    int reserve(size_t) const { return REDIO_OK; }
    hipError_t launch_fused(const void *, float *, long, bool, hipStream_t) const { return hipErrorNotSupported; }
    int spectra(const void *d_in, size_t g0, size_t, void *, const float2 *&spec) const
    {
        spec = (const float2 *)d_in + g0 * c.B;
        return REDIO_OK;
    }
};
int enqueue_spectra(Pspec &c, const void *d_spectra, size_t nbatch, void *d_out, void *stream)
{
    return enqueue(c, Spectra{c}, d_spectra, nbatch, nbatch / c.K, d_out, stream);
}
} // namespace

struct redio_pspec {
    Pspec c;
    bool packs;            // generic path: rows are gathered (window or step != N) before the transform, which then runs in place
    bool fft_stages;       // the plan's transform stages through a buffer of its own at this size (redio_fft_reserve)
    bool fft_stages_packed; // the same for a packed chunk transformed in place: what a u8 call runs on every plan (== fft_stages when packs)
    size_t packed_cap;     // transforms per pass for which the in-place transform's staging has been reserved
    bool fft_u8;           // the transform has a sibling that converts (and windows) bytes at its own load (2048, 4096): a u8 call needs no gather
    redio_fft *fft;
    void *d_rows;          // generic path: rows_cap rows of N cf32
    size_t rows_cap;
};

struct redio_pspec_real {
    Pspec c;
    bool packs;            // generic path: rows are always gathered (window or step != N); otherwise only a 4-byte aligned stream is
    redio_fftr *fftr;      // forward, size N: twiddles, super twiddles, the generic transform
    void *d_rows;          // generic path: rows_cap gathered rows of N f32
    size_t rows_cap;
    void *d_spec;          // generic path: spec_cap spectra of B cf32
    size_t spec_cap;
    size_t fftr_cap;       // rows per call the plan's redio_fftr has been reserved for
};

struct redio_pfb_pspec {
    Pspec c;               // nfft = M P samples per transform, B = M bins, step = M
    int M, P;
    redio_pfb *pfb;        // the channelizer: taps, table, and on the generic path the rows themselves
    void *d_rows;          // generic path: rows_cap channelizer rows of M cf32
    size_t rows_cap;
    size_t pfb_cap, pfb_cap_u8; // rows per pass the channelizer's own scratch has been reserved for, from cf32 and from bytes
};

namespace {
// cf32 samples in (redio_pspec_enqueue) and u8 I/Q byte pairs in (redio_pspec_enqueue_u8: one 16-bit word per sample, a sample-aligned
// pointer as the cf32 entry asks for 8).  U8 gathers rows and transforms them in place on every plan that has no launch_fft_u8.
template <bool U8>
struct Complex {
    redio_pspec *h;
    static constexpr bool transforms = true;
    static constexpr uintptr_t align = U8 ? 1 : 7;
    using Sample = std::conditional_t<U8, uint16_t, float2>;
    size_t in_bytes(size_t n_in) const { return n_in * sizeof(Sample); }
    bool stages() const { return U8 ? h->fft_stages_packed : h->fft_stages; }
    bool short_rows(size_t pass) const { return pass * (size_t)h->c.nfft > h->rows_cap || (U8 && stages() && pass > h->packed_cap); }
    int reserve(size_t pass) const
    {
        if (stages()) {
            if (int rc = redio_fft_reserve(h->fft, pass)) return rc;
            if ((U8 || h->packs) && pass > h->packed_cap) h->packed_cap = pass;
        }
        return scratch_grow(&h->d_rows, &h->rows_cap, pass * (size_t)h->c.nfft, sizeof(float2));
    }
    hipError_t launch_fused(const void *d_in, float *dst, long nunits, bool split, hipStream_t st) const
    {
        const Pspec &c = h->c;
        if constexpr (U8) return launch_pspec1k_u8((const uint16_t *)d_in, (long)c.step, (long)c.K, c.d_win, redio_fft_twiddles_dev(h->fft), dst, nunits, split, st);
        else return launch_pspec1k((const float2 *)d_in, (long)c.step, (long)c.K, c.d_win, redio_fft_twiddles_dev(h->fft), dst, nunits, split, st);
    }
    int spectra(const void *d_in, size_t g0, size_t ntr, void *stream, const float2 *&spec) const
    {
        const Pspec &c = h->c;
        const Sample *x = (const Sample *)d_in;
        const long N = c.nfft;
        hipStream_t st = (hipStream_t)stream;
        float2 *rows = (float2 *)h->d_rows;
        spec = rows;
        if constexpr (U8) {
            if (h->fft_u8) // the transform converts and windows at its own load: bytes in, spectra out
                return hip_rc(launch_fft_u8(*redio_fft_plan_dev(h->fft), x + g0 * c.step, c.d_win, rows, (long)ntr, (long)c.step, st));
            REDIO_TRY(launch_pspec_rows_u8(x + g0 * c.step, c.d_win, rows, (long)ntr, N, (long)c.step, st));
        } else {
            if (!h->packs) return redio_fft_enqueue(h->fft, x + g0 * (size_t)N, rows, ntr, stream);
            REDIO_TRY(launch_pspec_rows(x + g0 * c.step, c.d_win, rows, (long)ntr, N, (long)c.step, st));
        }
        return redio_fft_enqueue(h->fft, rows, rows, ntr, stream);
    }
};

// f32 samples in (redio_pspec_real_enqueue), 4-byte aligned
struct Real {
    redio_pspec_real *h;
    static constexpr bool transforms = true;
    static constexpr uintptr_t align = 3;
    size_t in_bytes(size_t n_in) const { return n_in * sizeof(float); }
    bool short_rows(size_t pass) const { return pass * (size_t)h->c.nfft > h->rows_cap || pass * h->c.B > h->spec_cap || pass > h->fftr_cap; }
    int reserve(size_t pass) const
    {
        if (pass > h->fftr_cap) {
            if (int rc = redio_fftr_reserve(h->fftr, pass)) return rc;
            h->fftr_cap = pass;
        }
        // the row scratch on every plan: a stream that is only 4-byte aligned is gathered even without a window at step == N
        if (int rc = scratch_grow(&h->d_rows, &h->rows_cap, pass * (size_t)h->c.nfft, sizeof(float))) return rc;
        return scratch_grow(&h->d_spec, &h->spec_cap, pass * h->c.B, sizeof(float2));
    }
    hipError_t launch_fused(const void *d_in, float *dst, long nunits, bool split, hipStream_t st) const
    {
        const Pspec &c = h->c;
        return launch_pspecr2k((const float *)d_in, (long)c.step, (long)c.K, c.d_win, redio_fftr_twiddles_dev(h->fftr), redio_fftr_super_dev(h->fftr), dst,
                               nunits, split, st);
    }
    int spectra(const void *d_in, size_t g0, size_t ntr, void *stream, const float2 *&spec) const
    {
        const Pspec &c = h->c;
        const float *x = (const float *)d_in;
        const long N = c.nfft;
        float2 *out = (float2 *)h->d_spec;
        spec = out;
        if (!h->packs && !((uintptr_t)d_in & 7)) // the transform reads its rows as cf32, 8-byte aligned, from the caller's buffer
            return redio_fftr_enqueue_strided(h->fftr, x + g0 * (size_t)N, out, ntr, N, (long)c.B, stream);
        float *rows = (float *)h->d_rows;
        REDIO_TRY(launch_pspec_real_rows(x + g0 * c.step, c.d_win, rows, (long)ntr, N, (long)c.step, (hipStream_t)stream));
        return redio_fftr_enqueue(h->fftr, rows, out, ntr, stream);
    }
};

// the polyphase spectrometer: cf32 samples in (redio_pfb_pspec_enqueue) or u8 I/Q byte pairs (redio_pfb_pspec_enqueue_u8).  A
// "transform" is one channelizer row; a pass of ntr rows reads (ntr + P - 1) M samples.
template <bool U8>
struct Polyphase {
    redio_pfb_pspec *h;
    static constexpr bool transforms = true;
    static constexpr uintptr_t align = U8 ? 1 : 7;
    using Sample = std::conditional_t<U8, uint16_t, float2>;
    size_t in_bytes(size_t n_in) const { return n_in * sizeof(Sample); }
    size_t pass_in(size_t pass) const { return (pass + (size_t)h->P - 1) * (size_t)h->M; }
    size_t &cap() const { return U8 ? h->pfb_cap_u8 : h->pfb_cap; }
    bool short_rows(size_t pass) const { return pass * (size_t)h->M > h->rows_cap || pass > cap(); }
    int reserve(size_t pass) const
    {
        if (pass > cap()) {
            if (int rc = U8 ? redio_pfb_reserve_u8(h->pfb, 2 * pass_in(pass), 1) : redio_pfb_reserve(h->pfb, pass_in(pass), 1)) return rc;
            cap() = pass;
        }
        return scratch_grow(&h->d_rows, &h->rows_cap, pass * (size_t)h->M, sizeof(float2));
    }
    hipError_t launch_fused(const void *d_in, float *dst, long nunits, bool split, hipStream_t st) const
    {
        const float *taps; const float2 *tw; unsigned flags; int fk;
        redio_pfb_tables(h->pfb, &taps, &tw, &flags, &fk);
        if (h->c.block)
            return launch_pfbspec_p2(d_in, U8, taps, tw, redio_pfb_twiddles_pass(h->pfb), dst, nunits, (long)h->c.K, h->M, h->P, split,
                                     (flags & REDIO_FIR_FUSED) != 0, st);
        return launch_pfbspec64(d_in, U8, taps, tw, dst, nunits, (long)h->c.K, h->P, split, (flags & REDIO_FIR_FUSED) != 0, st);
    }
    int spectra(const void *d_in, size_t g0, size_t ntr, void *stream, const float2 *&spec) const
    {
        const Sample *x = (const Sample *)d_in + g0 * (size_t)h->M;
        spec = (const float2 *)h->d_rows;
        if constexpr (U8) return redio_pfb_enqueue_u8(h->pfb, x, 2 * pass_in(ntr), h->d_rows, 1, stream);
        else return redio_pfb_enqueue(h->pfb, x, pass_in(ntr), h->d_rows, 1, stream);
    }
};
} // namespace

extern "C" int redio_pspec_create(redio_pspec **h, int nfft, size_t integrate, size_t step, const float *window_host)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (nfft < 1 || integrate == 0 || step == 0) return REDIO_ERR_ARG;
    redio_fft *fft = nullptr;
    if (int rc = redio_fft_create(&fft, nfft, 0)) return rc; // its own refusals: the size ceiling, no device
    redio_pspec *p = new (std::nothrow) redio_pspec();
    if (!p) { redio_fft_destroy(fft); return REDIO_ERR_NOMEM; }
    p->fft = fft;
    p->packs = window_host != nullptr || step != (size_t)nfft;
    p->fft_stages = redio_fft_stages(fft, p->packs); // a packed chunk is transformed in place
    p->fft_u8 = fft_u8_supported(*redio_fft_plan_dev(fft));
    p->fft_stages_packed = !p->fft_u8 && redio_fft_stages(fft, true);
    if (int rc = pspec_init(p->c, nfft, (size_t)nfft, integrate, step, nfft == 1024, PSPEC_SPLIT_ROWS, window_host)) {
        redio_pspec_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_pspec_real_create(redio_pspec_real **h, int nfft, size_t integrate, size_t step, const float *window_host)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (nfft < 2 || (nfft & 1) || integrate == 0 || step == 0) return REDIO_ERR_ARG;
    redio_fftr *fftr = nullptr;
    if (int rc = redio_fftr_create(&fftr, nfft, 0)) return rc; // its own refusals: the size ceiling, no device
    redio_pspec_real *p = new (std::nothrow) redio_pspec_real();
    if (!p) { redio_fftr_destroy(fftr); return REDIO_ERR_NOMEM; }
    p->fftr = fftr;
    p->packs = window_host != nullptr || step != (size_t)nfft;
    if (int rc = pspec_init(p->c, nfft, (size_t)nfft / 2 + 1, integrate, step, nfft == 2 * FFTR1K_M, PSPEC_REAL_SPLIT_ROWS, window_host)) {
        redio_pspec_real_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_pspec_destroy(redio_pspec *h)
{
    if (!h) return REDIO_OK;
    redio_fft_destroy(h->fft);
    pspec_free(h->c);
    redio_free(h->d_rows);
    delete h;
    return REDIO_OK;
}

extern "C" int redio_pspec_real_destroy(redio_pspec_real *h)
{
    if (!h) return REDIO_OK;
    redio_fftr_destroy(h->fftr);
    pspec_free(h->c);
    redio_free(h->d_rows); redio_free(h->d_spec);
    delete h;
    return REDIO_OK;
}

// the handle-typed faces of the shared functions
void redio_pspec_shape(const redio_pspec *h, int *nfft, size_t *K, size_t *step, int *device) { *nfft = h->c.nfft; *K = h->c.K; *step = h->c.step; *device = h->c.device; }
void redio_pspec_real_shape(const redio_pspec_real *h, int *nfft, size_t *K, size_t *step, int *device) { *nfft = h->c.nfft; *K = h->c.K; *step = h->c.step; *device = h->c.device; }
extern "C" size_t redio_pspec_nrows(const redio_pspec *h, size_t n_in) { return h ? nrows_of(h->c, n_in) : 0; }
extern "C" size_t redio_pspec_real_nrows(const redio_pspec_real *h, size_t n_in) { return h ? nrows_of(h->c, n_in) : 0; }
extern "C" size_t redio_pspec_real_nbins(const redio_pspec_real *h) { return h ? h->c.B : 0; }
extern "C" int redio_pspec_is_fused(const redio_pspec *h) { return h && h->c.fused ? 1 : 0; }
extern "C" int redio_pspec_real_is_fused(const redio_pspec_real *h) { return h && h->c.fused ? 1 : 0; }
extern "C" int redio_pspec_set_split(redio_pspec *h, int mode) { return h ? set_split(h->c, mode) : REDIO_ERR_ARG; }
extern "C" int redio_pspec_real_set_split(redio_pspec_real *h, int mode) { return h ? set_split(h->c, mode) : REDIO_ERR_ARG; }

extern "C" int redio_pspec_reserve(redio_pspec *h, size_t n_in)
{
    return h ? reserve(h->c, Complex<false>{h}, nrows_of(h->c, n_in)) : REDIO_ERR_ARG;
}
extern "C" int redio_pspec_reserve_u8(redio_pspec *h, size_t nbytes)
{
    return h ? reserve(h->c, Complex<true>{h}, nrows_of(h->c, nbytes / 2)) : REDIO_ERR_ARG;
}
extern "C" int redio_pspec_real_reserve(redio_pspec_real *h, size_t n_in)
{
    return h ? reserve(h->c, Real{h}, nrows_of(h->c, n_in)) : REDIO_ERR_ARG;
}

extern "C" int redio_pspec_enqueue(redio_pspec *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    return h ? enqueue(h->c, Complex<false>{h}, d_in, n_in, nrows_of(h->c, n_in), d_out, stream) : REDIO_ERR_ARG;
}
extern "C" int redio_pspec_enqueue_u8(redio_pspec *h, const void *d_bytes, size_t nbytes, void *d_out, void *stream)
{
    if (!h || (nbytes & 1)) return REDIO_ERR_ARG;
    return enqueue(h->c, Complex<true>{h}, d_bytes, nbytes / 2, nrows_of(h->c, nbytes / 2), d_out, stream);
}
extern "C" int redio_pspec_real_enqueue(redio_pspec_real *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    return h ? enqueue(h->c, Real{h}, d_in, n_in, nrows_of(h->c, n_in), d_out, stream) : REDIO_ERR_ARG;
}
extern "C" int redio_pspec_enqueue_spectra(redio_pspec *h, const void *d_spectra, size_t nbatch, void *d_out, void *stream)
{
    return h ? enqueue_spectra(h->c, d_spectra, nbatch, d_out, stream) : REDIO_ERR_ARG;
}
extern "C" int redio_pspec_real_enqueue_spectra(redio_pspec_real *h, const void *d_spectra, size_t nbatch, void *d_out, void *stream)
{
    return h ? enqueue_spectra(h->c, d_spectra, nbatch, d_out, stream) : REDIO_ERR_ARG;
}

// ---- the polyphase spectrometer (include/redio.h, redio_pfb_pspec_*) ----
extern "C" int redio_pfb_pspec_create(redio_pfb_pspec **h, const float *proto, int nchan, int taps_per_branch, size_t integrate, unsigned flags)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (integrate == 0) return REDIO_ERR_ARG;
    redio_pfb *pfb = nullptr;
    const bool want_block = (flags & REDIO_PFB_PSPEC_BLOCK) != 0; // this plan's own flag: the channelizer never sees it
    flags &= ~REDIO_PFB_PSPEC_BLOCK;
    if (int rc = redio_pfb_create(&pfb, proto, nchan, taps_per_branch, flags)) return rc; // its own refusals
    redio_pfb_pspec *p = new (std::nothrow) redio_pfb_pspec();
    if (!p) { redio_pfb_destroy(pfb); return REDIO_ERR_NOMEM; }
    p->pfb = pfb; p->M = nchan; p->P = taps_per_branch;
    const float *taps; const float2 *tw; unsigned fl; int fused;
    redio_pfb_tables(pfb, &taps, &tw, &fl, &fused);
    // the workgroup kernel where the caller asked for it and the channelizer has its one-kernel form (never 64 channels)
    const bool block = want_block && !fused && pfb_p2_supported(nchan, taps_per_branch);
    // auto mode: a wave per run of whole rows once those runs give PFBSPEC_SPLIT_WAVES waves; the workgroup kernel: a stream per
    // run of whole rows once those runs fill PFBSPEC_P2_SPLIT_GROUPS_PER_CU workgroups per CU (pfb_pspec_p2_core.h)
    const long split_rows = block ? pfbspec_p2_split_rows((long)integrate, num_cus(), nchan)
                                  : PFBSPEC_SPLIT_WAVES * pfbspec_units_per_wave(1, (long)integrate, false);
    p->c.block = block;
    if (int rc = pspec_init(p->c, nchan * taps_per_branch, (size_t)nchan, integrate, (size_t)nchan, fused != 0, split_rows, nullptr)) {
        redio_pfb_pspec_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}
extern "C" int redio_pfb_pspec_destroy(redio_pfb_pspec *h)
{
    if (!h) return REDIO_OK;
    redio_pfb_destroy(h->pfb);
    pspec_free(h->c);
    redio_free(h->d_rows);
    delete h;
    return REDIO_OK;
}
void redio_pfb_pspec_shape(const redio_pfb_pspec *h, int *window, size_t *K, size_t *step, int *device) { *window = h->c.nfft; *K = h->c.K; *step = h->c.step; *device = h->c.device; }
extern "C" size_t redio_pfb_pspec_nrows(const redio_pfb_pspec *h, size_t n_in) { return h ? nrows_of(h->c, n_in) : 0; }
extern "C" int redio_pfb_pspec_is_fused(const redio_pfb_pspec *h) { return h && h->c.fused ? 1 : 0; }
extern "C" int redio_pfb_pspec_route(const redio_pfb_pspec *h) { return !h ? 0 : h->c.block ? 2 : h->c.fused ? 1 : 0; }
extern "C" int redio_pfb_pspec_set_split(redio_pfb_pspec *h, int mode) { return h ? set_split(h->c, mode) : REDIO_ERR_ARG; }
extern "C" int redio_pfb_pspec_reserve(redio_pfb_pspec *h, size_t n_in)
{
    return h ? reserve(h->c, Polyphase<false>{h}, nrows_of(h->c, n_in)) : REDIO_ERR_ARG;
}
extern "C" int redio_pfb_pspec_reserve_u8(redio_pfb_pspec *h, size_t nbytes)
{
    return h ? reserve(h->c, Polyphase<true>{h}, nrows_of(h->c, nbytes / 2)) : REDIO_ERR_ARG;
}
extern "C" int redio_pfb_pspec_enqueue(redio_pfb_pspec *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    return h ? enqueue(h->c, Polyphase<false>{h}, d_in, n_in, nrows_of(h->c, n_in), d_out, stream) : REDIO_ERR_ARG;
}
extern "C" int redio_pfb_pspec_enqueue_u8(redio_pfb_pspec *h, const void *d_bytes, size_t nbytes, void *d_out, void *stream)
{
    if (!h || (nbytes & 1)) return REDIO_ERR_ARG;
    return enqueue(h->c, Polyphase<true>{h}, d_bytes, nbytes / 2, nrows_of(h->c, nbytes / 2), d_out, stream);
}
