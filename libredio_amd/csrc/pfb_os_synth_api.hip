// pfb_os_synth_api.hip -- C ABI of the oversampled synthesis bank plan (include/redio_pfb_os_synth.h, redio_pfb_os_synth_*).
//
// The way back from the oversampled channelizer's rows: inverse transform of every row, then a weighted overlap-add at hop H <= M.
// Route 1 (64 channels, hop 32, 4 / 8 / 16 taps per branch): pfb_os_synth_kernels.hip, one kernel, no scratch.
// Route 0 (every other shape, and route-1 shapes after set_unfused): the plan's own inverse redio_fft over the rows into plan-owned
// scratch, then the overlap-add pass (pfb_os_synth_kernels.hip, one thread per output sample) -- in chunks of at most 64 MiB of whole
// rows whose edges overlap by L - 1 rows; a chunk's first_row advances by the rows before it.  The same bits on both routes.  The
// carried-history stream (redio_pfb_os_synth_stream_*) is stream_carry.hip's, like every other plan's.
#include "../../include/redio.h"
#include "pfb_os_synth_core.h"
#include "redio_internal.h"
#include <new>

namespace redio {
bool pfb_os_synth_supported(int nchan, int taps_per_branch, size_t hop);
hipError_t launch_pfb_os_synth(const float2 *x, const float *h, const float2 *tw64_inv, float2 *out, long hops, int taps_per_branch, uint64_t first_row,
                               bool fused, hipStream_t s);
hipError_t launch_pfb_os_synth_ola(const float2 *w, const float *h, float2 *out, long hops, int M, int P, long H, long f0, bool fused, hipStream_t st);
} // namespace redio
using namespace redio;

struct redio_pfb_os_synth {
    int device, M, P;
    size_t H, L;         // hop, and rows per output hop: ceil(M P / H)
    unsigned flags;
    float *d_h;          // the prototype, M P taps
    redio_fft *fft;      // the M-point INVERSE plan: route 0's first pass, and route 1's twiddle table
    bool wave_kernel;    // the shape has the one-kernel form
    int force_unfused;   // redio_pfb_os_synth_set_unfused
    size_t chunk_rows;   // route 0: input rows per pass through the scratch (at least L)
    void *d_v;           // route 0: v_cap transformed rows of M cf32
    size_t v_cap;
    bool fft_stages;     // the transform stages through a buffer of its own at this size (redio_fft_reserve)
    size_t fft_cap;      // rows per call it has been reserved for
};

static size_t oss_default_chunk(const redio_pfb_os_synth *h)
{
    const size_t rows = ((size_t)64 << 20) / ((size_t)h->M * sizeof(float2));
    return rows < h->L ? h->L : rows;
}

extern "C" int redio_pfb_os_synth_create(redio_pfb_os_synth **h, const float *proto, int nchan, int taps_per_branch, size_t hop, unsigned flags)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!proto || nchan <= 0 || taps_per_branch <= 0) return REDIO_ERR_ARG; // what redio_pfb_create refuses
    if (hop == 0 || hop > (size_t)nchan) return REDIO_ERR_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_pfb_os_synth *p = new (std::nothrow) redio_pfb_os_synth();
    if (!p) return REDIO_ERR_NOMEM;
    p->device = dev; p->M = nchan; p->P = taps_per_branch; p->H = hop; p->flags = flags;
    p->L = (size_t)pfboss_L(nchan, taps_per_branch, (long)hop);
    p->wave_kernel = pfb_os_synth_supported(nchan, taps_per_branch, hop);
    p->chunk_rows = oss_default_chunk(p);
    int rc = redio_fft_create(&p->fft, nchan, 1);
    const size_t nt = (size_t)nchan * taps_per_branch;
    if (rc == REDIO_OK) rc = hip_rc(hipMalloc((void **)&p->d_h, nt * sizeof(float)));
    if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(p->d_h, proto, nt * sizeof(float), hipMemcpyHostToDevice));
    if (rc != REDIO_OK) { redio_pfb_os_synth_destroy(p); return rc; }
    p->fft_stages = redio_fft_stages(p->fft, false);
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_pfb_os_synth_destroy(redio_pfb_os_synth *h)
{
    if (!h) return REDIO_OK;
    hipFree(h->d_h);
    redio_free(h->d_v);
    redio_fft_destroy(h->fft);
    delete h;
    return REDIO_OK;
}

void redio_pfb_os_synth_shape(const redio_pfb_os_synth *h, int *nchan, int *taps_per_branch, size_t *hop, int *device)
{
    *nchan = h->M; *taps_per_branch = h->P; *hop = h->H; *device = h->device;
}

extern "C" size_t redio_pfb_os_synth_nout(const redio_pfb_os_synth *h, size_t n_in)
{
    if (!h) return 0;
    const size_t T = n_in / (size_t)h->M;
    return T < h->L ? 0 : (T - h->L + 1) * h->H;
}
extern "C" size_t redio_pfb_os_synth_hop(const redio_pfb_os_synth *h) { return h ? h->H : 0; }
extern "C" int redio_pfb_os_synth_route(const redio_pfb_os_synth *h) { return h && h->wave_kernel && !h->force_unfused ? 1 : 0; }
extern "C" int redio_pfb_os_synth_is_fused(const redio_pfb_os_synth *h) { return redio_pfb_os_synth_route(h); }
extern "C" int redio_pfb_os_synth_set_unfused(redio_pfb_os_synth *h, int unfused)
{
    if (!h) return REDIO_ERR_ARG;
    h->force_unfused = unfused ? 1 : 0;
    return REDIO_OK;
}
// tests and measurement: input rows per pass of route 0 (0: the default, 64 MiB of rows); fewer than L rows count as L
extern "C" int redio_pfb_os_synth_set_chunk_rows(redio_pfb_os_synth *h, size_t rows)
{
    if (!h) return REDIO_ERR_ARG;
    h->chunk_rows = rows == 0 ? oss_default_chunk(h) : rows < h->L ? h->L : rows;
    return REDIO_OK;
}

// input rows of the largest pass of a call with T input rows
static size_t oss_pass_rows(const redio_pfb_os_synth *h, size_t T) { return T < h->chunk_rows ? T : h->chunk_rows; }

extern "C" int redio_pfb_os_synth_reserve(redio_pfb_os_synth *h, size_t n_in)
{
    if (!h) return REDIO_ERR_ARG;
    if (redio_pfb_os_synth_route(h) == 1) return REDIO_OK;
    const size_t T = n_in / (size_t)h->M;
    if (T < h->L) return REDIO_OK;
    const size_t pass = oss_pass_rows(h, T);
    REDIO_TRY(hipSetDevice(h->device));
    if (int rc = scratch_grow(&h->d_v, &h->v_cap, pass * (size_t)h->M, sizeof(float2))) return rc;
    if (h->fft_stages && pass > h->fft_cap) {
        if (int rc = redio_fft_reserve(h->fft, pass)) return rc;
        h->fft_cap = pass;
    }
    return REDIO_OK;
}

extern "C" int redio_pfb_os_synth_enqueue(redio_pfb_os_synth *h, const void *d_in, size_t n_in, uint64_t first_row, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t M = (size_t)h->M, H = h->H, L = h->L;
    const size_t nout = redio_pfb_os_synth_nout(h, n_in);
    if (nout == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return REDIO_ERR_ARG;
    const size_t T = n_in / M, hops = nout / H;
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + nout * sizeof(float2) && o < a + T * M * sizeof(float2)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const bool fused = (h->flags & REDIO_FIR_FUSED) != 0;
    if (redio_pfb_os_synth_route(h) == 1) {
        const hipError_t e = launch_pfb_os_synth((const float2 *)d_in, h->d_h, redio_fft_twiddles_dev(h->fft), (float2 *)d_out, (long)hops, h->P, first_row, fused, st);
        return e == hipErrorNotSupported ? REDIO_ERR_UNSUPPORTED : hip_rc(e);
    }
    const size_t pass = oss_pass_rows(h, T);
    if (pass * M > h->v_cap || (h->fft_stages && pass > h->fft_cap)) { // un-reserved: grow on first use, never inside a capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = redio_pfb_os_synth_reserve(h, n_in)) return rc;
    }
    // hops [c0, c0 + n) come from input rows [c0, c0 + n + L - 1): consecutive passes overlap by L - 1 input rows
    const size_t per = pass - L + 1;
    for (size_t c0 = 0; c0 < hops; c0 += per) {
        const size_t n = hops - c0 < per ? hops - c0 : per;
        const long f0 = (long)((first_row + (uint64_t)c0) % (uint64_t)M); // F + T does not pass 2^64
        if (int rc = redio_fft_enqueue(h->fft, (const float2 *)d_in + c0 * M, h->d_v, n + L - 1, stream)) return rc;
        REDIO_TRY(launch_pfb_os_synth_ola((const float2 *)h->d_v, h->d_h, (float2 *)d_out + c0 * H, (long)n, h->M, h->P, (long)H, f0, fused, st));
    }
    return REDIO_OK;
}
