// pfb_bank.hip -- C ABI of the three two-pass filterbank plans: the synthesis bank (include/redio.h, redio_pfb_synth_*), the oversampled
// channelizer (redio_pfb_os_*) and the oversampled synthesis bank (include/redio_pfb_os_synth.h, redio_pfb_os_synth_*).
//
// One driver.  A plan is an M-point redio_fft and a filter pass over rows of M cf32, in either order:
//     synthesis bank              inverse transform, then the channelizer's branch filter (pfb_api.hip, launch_pfb_branch)
//     oversampled channelizer     branch filter at row stride H with a rotated store (pfb_os_kernels.hip), then forward transform
//     oversampled synthesis bank  inverse transform, then the weighted overlap-add at hop H (pfb_os_synth_kernels.hip)
// Route 1 (64 channels x 4 / 8 / 16 taps per branch; the oversampled plans at hop 32): the family's wave kernel, one launch, no scratch.
// Route 2 (the oversampled channelizer with REDIO_PFB_OS_BLOCK: 32 ... 1024 channels at hop M / 2, pfb_os_p2.hip): the family's workgroup
// kernel, one launch, no scratch.
// Route 0 (every other shape, and route-1 and route-2 shapes after set_unfused): the two passes through plan-owned scratch, in chunks of
// at most 64 MiB of rows cut by pfb_bank_cut.h; a chunk's first_row advances by the units before it.  The same bits on every route.
// What tells the families apart is data: BankFamily (direction and order of the transform, the launchers) and the plan's BankCut
// (window, hop, output per unit, rows a pass needs at least).  The driver never asks which family it serves.  Each family's own code is
// its create entry (arguments, which cut of pfb_bank_cut.h, "is there a wave kernel"), its shape function and the signature of its enqueue.
// The carried-history streams (redio_*_stream_*) are stream_carry.hip's, like every other plan's.
#include "../../include/redio.h"
#include "pfb_bank_cut.h"
#include "redio_internal.h"
#include <new>

namespace redio {
bool pfb_synth_supported(int nchan, int taps_per_branch);
bool pfb_os_supported(int nchan, int taps_per_branch, size_t hop);
bool pfb_os_synth_supported(int nchan, int taps_per_branch, size_t hop);
hipError_t launch_pfb_synth(const float2 *x, const float *h, const float2 *tw64_inv, float2 *out, long rows, int taps_per_branch, bool fused, hipStream_t s);
hipError_t launch_pfb_branch(const float2 *x, const float *h, float2 *v, long rows, int M, int P, bool fused, hipStream_t st); // pfb_api.hip
// the common signatures.  Wave kernel: `units` units from x into out.  Filter pass: `units` units from `in` (the stream, or the scratch
// behind the transform) into `out` (the scratch in front of the transform, or the output); f0 = (F + the pass's first unit) mod M
typedef hipError_t BankWaveFn(const float2 *x, const float *h, const float2 *tw64, float2 *out, long units, int taps_per_branch, uint64_t first_row,
                              bool fused, hipStream_t s);
typedef hipError_t BankFilterFn(const float2 *in, const float *h, float2 *out, long units, int M, int P, long H, long f0, bool fused, hipStream_t st);
// Workgroup kernel: `units` units from x into out; tw: the M-entry table, Tord: the 512-point plan's stage-ordered copy (else null)
typedef hipError_t BankBlockFn(const float2 *x, const float *h, const float2 *tw, const float2 *Tord, float2 *out, long units, int M, int P,
                               uint64_t first_row, bool fused, hipStream_t s);
bool pfb_os_p2_supported(int nchan, int taps_per_branch, size_t hop);
BankBlockFn launch_pfb_os_p2;                                 // pfb_os_p2.hip
BankWaveFn launch_pfb_os, launch_pfb_os_synth;                // pfb_os_kernels.hip, pfb_os_synth_kernels.hip
BankFilterFn launch_pfb_os_synth_ola;                         // pfb_os_synth_kernels.hip
__attribute__((visibility("hidden"))) BankFilterFn launch_pfb_os_branch; // pfb_os_kernels.hip; not in the exported symbol set
} // namespace redio
using namespace redio;

namespace {
// the synthesis bank has no row index and no hop of its own
hipError_t synth_wave(const float2 *x, const float *h, const float2 *tw, float2 *out, long units, int P, uint64_t, bool fused, hipStream_t s)
{
    return launch_pfb_synth(x, h, tw, out, units, P, fused, s);
}
hipError_t synth_filter(const float2 *in, const float *h, float2 *out, long units, int M, int P, long, long, bool fused, hipStream_t st)
{
    return launch_pfb_branch(in, h, out, units, M, P, fused, st);
}

struct BankFamily {
    int inverse;          // the direction of the plan's redio_fft
    bool transform_first; // route 0: transform into the scratch, then filter; or filter into the scratch, then transform
    BankWaveFn *wave;
    BankFilterFn *filter;
    BankBlockFn *block;   // route 2's kernel; null: the family has none
};
const BankFamily SYNTH = {1, true, synth_wave, synth_filter, nullptr};
const BankFamily OS = {0, false, launch_pfb_os, launch_pfb_os_branch, launch_pfb_os_p2};
const BankFamily OS_SYNTH = {1, true, launch_pfb_os_synth, launch_pfb_os_synth_ola, nullptr};
} // namespace

struct redio_pfb_bank {
    const BankFamily *fam;
    BankCut cut;
    int device, M, P;
    size_t H;            // the hop the filter pass is told (the synthesis bank: M)
    unsigned flags;
    float *d_h;          // the prototype, M P taps
    redio_fft *fft;      // the M-point plan: one of route 0's passes, and route 1's twiddle table
    bool wave_kernel;    // the shape has the one-kernel form
    bool block_kernel;   // the plan asked for the workgroup form and the shape has it (route 2)
    int force_unfused;   // set_unfused
    size_t chunk_rows;   // route 0: scratch rows per pass (at least cut.min_rows)
    void *d_v;           // route 0: v_cap elements, a pass's rows between the two passes
    size_t v_cap;
    bool fft_stages;     // the transform stages through a buffer of its own at this size (redio_fft_reserve)
    size_t fft_cap;      // rows per call it has been reserved for
};
struct redio_pfb_synth : redio_pfb_bank {};
struct redio_pfb_os : redio_pfb_bank {};
struct redio_pfb_os_synth : redio_pfb_bank {};

static void bank_release(redio_pfb_bank *h)
{
    hipFree(h->d_h);
    redio_free(h->d_v);
    redio_fft_destroy(h->fft);
}

template <typename Hd>
static int bank_create(Hd **h, const BankFamily &fam, const float *proto, int nchan, int taps_per_branch, size_t hop, unsigned flags,
                       BankCut (*cut)(size_t M, size_t P, size_t H), bool wave_kernel, bool block_kernel = false)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!proto || nchan <= 0 || taps_per_branch <= 0) return REDIO_ERR_ARG; // what redio_pfb_create refuses
    if (hop == 0 || hop > (size_t)nchan) return REDIO_ERR_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    Hd *p = new (std::nothrow) Hd();
    if (!p) return REDIO_ERR_NOMEM;
    p->fam = &fam; p->cut = cut((size_t)nchan, (size_t)taps_per_branch, hop);
    p->device = dev; p->M = nchan; p->P = taps_per_branch; p->H = hop; p->flags = flags;
    p->wave_kernel = wave_kernel;
    p->block_kernel = block_kernel && fam.block && !wave_kernel;
    p->chunk_rows = bank_chunk_rows(p->cut, 0);
    int rc = redio_fft_create(&p->fft, nchan, fam.inverse);
    const size_t nt = (size_t)nchan * taps_per_branch;
    if (rc == REDIO_OK) rc = hip_rc(hipMalloc((void **)&p->d_h, nt * sizeof(float)));
    if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(p->d_h, proto, nt * sizeof(float), hipMemcpyHostToDevice));
    if (rc != REDIO_OK) { bank_release(p); delete p; return rc; }
    p->fft_stages = redio_fft_stages(p->fft, false);
    *h = p;
    return REDIO_OK;
}

static int bank_route(const redio_pfb_bank *h)
{
    if (!h || h->force_unfused) return 0;
    return h->wave_kernel ? 1 : h->block_kernel ? 2 : 0;
}

static int bank_reserve(redio_pfb_bank *h, size_t n_in)
{
    if (!h) return REDIO_ERR_ARG;
    if (bank_route(h) != 0) return REDIO_OK; // one launch, no scratch
    const size_t units = bank_units(h->cut, n_in);
    if (units == 0) return REDIO_OK;
    const size_t pass = bank_pass_rows(h->cut, h->chunk_rows, units);
    REDIO_TRY(hipSetDevice(h->device));
    if (int rc = scratch_grow(&h->d_v, &h->v_cap, pass * (size_t)h->M, sizeof(float2))) return rc;
    if (h->fft_stages && pass > h->fft_cap) {
        if (int rc = redio_fft_reserve(h->fft, pass)) return rc;
        h->fft_cap = pass;
    }
    return REDIO_OK;
}

static int bank_enqueue(redio_pfb_bank *h, const void *d_in, size_t n_in, uint64_t first_row, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const BankCut &c = h->cut;
    const BankFamily &fam = *h->fam;
    const size_t units = bank_units(c, n_in);
    if (units == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return REDIO_ERR_ARG;
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + units * c.unit_out * sizeof(float2) && o < a + bank_input(c, units) * sizeof(float2)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const bool fused = (h->flags & REDIO_FIR_FUSED) != 0;
    if (bank_route(h) == 1) {
        const hipError_t e = fam.wave((const float2 *)d_in, h->d_h, redio_fft_twiddles_dev(h->fft), (float2 *)d_out, (long)units, h->P, first_row, fused, st);
        return e == hipErrorNotSupported ? REDIO_ERR_UNSUPPORTED : hip_rc(e);
    }
    if (bank_route(h) == 2) {
        const hipError_t e = fam.block((const float2 *)d_in, h->d_h, redio_fft_twiddles_dev(h->fft), redio_fft_twiddles_pass_dev(h->fft), (float2 *)d_out,
                                       (long)units, h->M, h->P, first_row, fused, st);
        return e == hipErrorNotSupported ? REDIO_ERR_UNSUPPORTED : hip_rc(e);
    }
    const size_t pass = bank_pass_rows(c, h->chunk_rows, units);
    if (pass * (size_t)h->M > h->v_cap || (h->fft_stages && pass > h->fft_cap)) { // un-reserved: grow on first use, never inside a capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = bank_reserve(h, n_in)) return rc;
    }
    float2 *v = (float2 *)h->d_v;
    for (size_t i = 0, np = bank_passes(c, h->chunk_rows, units); i < np; ++i) {
        const BankPass p = bank_pass(c, h->chunk_rows, units, i);
        const float2 *in = (const float2 *)d_in + p.in_off;
        float2 *out = (float2 *)d_out + p.out_off;
        const long f0 = (long)((first_row + (uint64_t)p.first) % (uint64_t)h->M); // F + unit is taken modulo 2^64
        if (fam.transform_first) {
            if (int rc = redio_fft_enqueue(h->fft, in, v, p.rows, stream)) return rc;
            REDIO_TRY(fam.filter(v, h->d_h, out, (long)p.units, h->M, h->P, (long)h->H, f0, fused, st));
        } else {
            REDIO_TRY(fam.filter(in, h->d_h, v, (long)p.units, h->M, h->P, (long)h->H, f0, fused, st));
            if (int rc = redio_fft_enqueue(h->fft, v, out, p.rows, stream)) return rc;
        }
    }
    return REDIO_OK;
}

// what every family exports under its own prefix; set_chunk_rows is for tests and measurement: scratch rows per pass of route 0
// (0: the default, 64 MiB of rows; fewer than a pass needs count as that many)
#define RD_BANK_API(NAME)                                                                                                 \
    extern "C" int redio_##NAME##_destroy(redio_##NAME *h)                                                                \
    {                                                                                                                     \
        if (!h) return REDIO_OK;                                                                                          \
        bank_release(h);                                                                                                  \
        delete h;                                                                                                         \
        return REDIO_OK;                                                                                                  \
    }                                                                                                                     \
    extern "C" int redio_##NAME##_route(const redio_##NAME *h) { return bank_route(h); }                                  \
    extern "C" int redio_##NAME##_is_fused(const redio_##NAME *h) { return bank_route(h) == 1; }                          \
    extern "C" int redio_##NAME##_set_unfused(redio_##NAME *h, int unfused)                                               \
    {                                                                                                                     \
        if (!h) return REDIO_ERR_ARG;                                                                                     \
        h->force_unfused = unfused ? 1 : 0;                                                                               \
        return REDIO_OK;                                                                                                  \
    }                                                                                                                     \
    extern "C" int redio_##NAME##_set_chunk_rows(redio_##NAME *h, size_t rows)                                            \
    {                                                                                                                     \
        if (!h) return REDIO_ERR_ARG;                                                                                     \
        h->chunk_rows = bank_chunk_rows(h->cut, rows);                                                                    \
        return REDIO_OK;                                                                                                  \
    }                                                                                                                     \
    extern "C" int redio_##NAME##_reserve(redio_##NAME *h, size_t n_in) { return bank_reserve(h, n_in); }
RD_BANK_API(pfb_synth)
RD_BANK_API(pfb_os)
RD_BANK_API(pfb_os_synth)

// ---- the synthesis bank: a unit is an output row of M samples, from P rows of M channel values ----
extern "C" int redio_pfb_synth_create(redio_pfb_synth **h, const float *proto, int nchan, int taps_per_branch, unsigned flags)
{
    return bank_create(h, SYNTH, proto, nchan, taps_per_branch, (size_t)nchan, flags,
                       bank_cut_synth, pfb_synth_supported(nchan, taps_per_branch));
}
void redio_pfb_synth_shape(const redio_pfb_synth *h, int *nchan, int *taps_per_branch, int *device) { *nchan = h->M; *taps_per_branch = h->P; *device = h->device; }
extern "C" size_t redio_pfb_synth_nout(const redio_pfb_synth *h, size_t n_in) { return h ? bank_units(h->cut, n_in) * h->cut.unit_out : 0; }
extern "C" int redio_pfb_synth_enqueue(redio_pfb_synth *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    return bank_enqueue(h, d_in, n_in, 0, d_out, stream);
}

// ---- the oversampled channelizer: a unit is a row of M channels, from the M P samples that start every H ----
extern "C" int redio_pfb_os_create(redio_pfb_os **h, const float *proto, int nchan, int taps_per_branch, size_t hop, unsigned flags)
{
    const bool want_block = (flags & REDIO_PFB_OS_BLOCK) != 0; // this plan's own flag
    return bank_create(h, OS, proto, nchan, taps_per_branch, hop, flags & ~REDIO_PFB_OS_BLOCK,
                       bank_cut_os, pfb_os_supported(nchan, taps_per_branch, hop), want_block && pfb_os_p2_supported(nchan, taps_per_branch, hop));
}
void redio_pfb_os_shape(const redio_pfb_os *h, int *nchan, int *taps_per_branch, size_t *hop, int *device)
{
    *nchan = h->M; *taps_per_branch = h->P; *hop = h->H; *device = h->device;
}
extern "C" size_t redio_pfb_os_nrows(const redio_pfb_os *h, size_t n_in) { return h ? bank_units(h->cut, n_in) : 0; }
extern "C" size_t redio_pfb_os_hop(const redio_pfb_os *h) { return h ? h->H : 0; }
extern "C" int redio_pfb_os_enqueue(redio_pfb_os *h, const void *d_in, size_t n_in, uint64_t first_row, void *d_out, void *stream)
{
    return bank_enqueue(h, d_in, n_in, first_row, d_out, stream);
}

// ---- the oversampled synthesis bank: a unit is a hop of H samples, from L = ceil(M P / H) rows of M channel values ----
extern "C" int redio_pfb_os_synth_create(redio_pfb_os_synth **h, const float *proto, int nchan, int taps_per_branch, size_t hop, unsigned flags)
{
    return bank_create(h, OS_SYNTH, proto, nchan, taps_per_branch, hop, flags,
                       bank_cut_os_synth, pfb_os_synth_supported(nchan, taps_per_branch, hop));
}
void redio_pfb_os_synth_shape(const redio_pfb_os_synth *h, int *nchan, int *taps_per_branch, size_t *hop, int *device)
{
    *nchan = h->M; *taps_per_branch = h->P; *hop = h->H; *device = h->device;
}
extern "C" size_t redio_pfb_os_synth_nout(const redio_pfb_os_synth *h, size_t n_in) { return h ? bank_units(h->cut, n_in) * h->cut.unit_out : 0; }
extern "C" size_t redio_pfb_os_synth_hop(const redio_pfb_os_synth *h) { return h ? h->H : 0; }
extern "C" int redio_pfb_os_synth_enqueue(redio_pfb_os_synth *h, const void *d_in, size_t n_in, uint64_t first_row, void *d_out, void *stream)
{
    return bank_enqueue(h, d_in, n_in, first_row, d_out, stream);
}
