// pfb_os_api.hip -- C ABI of the oversampled channelizer plan (include/redio.h, redio_pfb_os_*).
//
// The channelizer with a hop H <= M between rows: branch filter on the M P samples from r H on, a circular shift of the branch sums by
// s_r = ((F + r) H) mod M, forward transform.
// Route 1 (64 channels, hop 32, 4 / 8 / 16 taps per branch): pfb_os_kernels.hip, one kernel, no scratch.
// Route 0 (every other shape, and route-1 shapes after set_unfused): the branch pass below (row stride H, rotated store) into plan-owned
// scratch, then the plan's own forward redio_fft over those rows into the output -- in chunks of at most 64 MiB of whole rows.  The same
// bits on both routes.  The carried-history stream (redio_pfb_os_stream_*) is stream_carry.hip's, like every other plan's.
#include "../../include/redio.h"
#include "pfb_os_core.h"
#include "redio_internal.h"
#include <new>

namespace redio {
bool pfb_os_supported(int nchan, int taps_per_branch, size_t hop);
hipError_t launch_pfb_os(const float2 *x, const float *h, const float2 *tw64, float2 *out, long rows, int taps_per_branch, uint64_t first_row, bool fused,
                         hipStream_t s);

// pfb_branch_kernel (pfb_api.hip) with a row stride of H: v[r][(m + s_r) mod M] = fold_p x[r H + p M + m] * h[M p + m] (ascending p, the
// reference's fold).  Rows H apart share samples only where H divides a multiple of M, so a thread is one (row, branch) and walks its P
// taps; consecutive threads are consecutive m (coalesced loads; the store is two coalesced runs, split where the rotation wraps).
// f0 = (F + the pass's first row) mod M.
template <bool FUSED>
__global__ __launch_bounds__(256) void pfb_os_branch_kernel(const float2 *__restrict__ x, const float *__restrict__ h, float2 *__restrict__ v, long rows,
                                                            int M, int P, long H, long f0)
{
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= rows * M) return;
    const long r = e / M;
    const int m = (int)(e - r * M);
    const float2 *col = x + r * H + m;
    float2 acc = make_float2(0.f, 0.f);
    for (int p = 0; p < P; ++p) acc = mac<FUSED>(col[(long)p * M], h[(long)p * M + m], acc);
    v[r * M + pfbos_rot(m, pfbos_shift(f0, r, M, H), M)] = acc;
}

static hipError_t launch_pfb_os_branch(const float2 *x, const float *h, float2 *v, long rows, int M, int P, long H, long f0, bool fused, hipStream_t st)
{
    if (rows <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((rows * M + 255) / 256);
    if (fused) hipLaunchKernelGGL(pfb_os_branch_kernel<true>, dim3(grid), dim3(256), 0, st, x, h, v, rows, M, P, H, f0);
    else hipLaunchKernelGGL(pfb_os_branch_kernel<false>, dim3(grid), dim3(256), 0, st, x, h, v, rows, M, P, H, f0);
    return hipGetLastError();
}
} // namespace redio
using namespace redio;

struct redio_pfb_os {
    int device, M, P;
    size_t H;
    unsigned flags;
    float *d_h;          // the prototype, M P taps
    redio_fft *fft;      // the M-point forward plan: route 0's second pass, and route 1's twiddle table
    bool wave_kernel;    // the shape has the one-kernel form
    int force_unfused;   // redio_pfb_os_set_unfused
    size_t chunk_rows;   // route 0: rows per pass through the scratch (at least 1)
    void *d_v;           // route 0: v_cap elements, the rotated branch sums of a pass
    size_t v_cap;
    bool fft_stages;     // the transform stages through a buffer of its own at this size (redio_fft_reserve)
    size_t fft_cap;      // rows per call it has been reserved for
};

static size_t os_default_chunk(const redio_pfb_os *h)
{
    const size_t rows = ((size_t)64 << 20) / ((size_t)h->M * sizeof(float2));
    return rows < 1 ? 1 : rows;
}

extern "C" int redio_pfb_os_create(redio_pfb_os **h, const float *proto, int nchan, int taps_per_branch, size_t hop, unsigned flags)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!proto || nchan <= 0 || taps_per_branch <= 0) return REDIO_ERR_ARG; // what redio_pfb_create refuses
    if (hop == 0 || hop > (size_t)nchan) return REDIO_ERR_ARG;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_pfb_os *p = new (std::nothrow) redio_pfb_os();
    if (!p) return REDIO_ERR_NOMEM;
    p->device = dev; p->M = nchan; p->P = taps_per_branch; p->H = hop; p->flags = flags;
    p->wave_kernel = pfb_os_supported(nchan, taps_per_branch, hop);
    p->chunk_rows = os_default_chunk(p);
    int rc = redio_fft_create(&p->fft, nchan, 0);
    const size_t nt = (size_t)nchan * taps_per_branch;
    if (rc == REDIO_OK) rc = hip_rc(hipMalloc((void **)&p->d_h, nt * sizeof(float)));
    if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(p->d_h, proto, nt * sizeof(float), hipMemcpyHostToDevice));
    if (rc != REDIO_OK) { redio_pfb_os_destroy(p); return rc; }
    p->fft_stages = redio_fft_stages(p->fft, false);
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_pfb_os_destroy(redio_pfb_os *h)
{
    if (!h) return REDIO_OK;
    hipFree(h->d_h);
    redio_free(h->d_v);
    redio_fft_destroy(h->fft);
    delete h;
    return REDIO_OK;
}

void redio_pfb_os_shape(const redio_pfb_os *h, int *nchan, int *taps_per_branch, size_t *hop, int *device)
{
    *nchan = h->M; *taps_per_branch = h->P; *hop = h->H; *device = h->device;
}

extern "C" size_t redio_pfb_os_nrows(const redio_pfb_os *h, size_t n_in)
{
    if (!h) return 0;
    const size_t W = (size_t)h->M * (size_t)h->P;
    return n_in < W ? 0 : (n_in - W) / h->H + 1;
}
extern "C" size_t redio_pfb_os_hop(const redio_pfb_os *h) { return h ? h->H : 0; }
extern "C" int redio_pfb_os_route(const redio_pfb_os *h) { return h && h->wave_kernel && !h->force_unfused ? 1 : 0; }
extern "C" int redio_pfb_os_is_fused(const redio_pfb_os *h) { return redio_pfb_os_route(h); }
extern "C" int redio_pfb_os_set_unfused(redio_pfb_os *h, int unfused)
{
    if (!h) return REDIO_ERR_ARG;
    h->force_unfused = unfused ? 1 : 0;
    return REDIO_OK;
}
// tests and measurement: rows per pass of route 0 (0: the default, 64 MiB of rows)
extern "C" int redio_pfb_os_set_chunk_rows(redio_pfb_os *h, size_t rows)
{
    if (!h) return REDIO_ERR_ARG;
    h->chunk_rows = rows == 0 ? os_default_chunk(h) : rows;
    return REDIO_OK;
}

// rows of the largest pass of a call with `rows` rows
static size_t os_pass_rows(const redio_pfb_os *h, size_t rows) { return rows < h->chunk_rows ? rows : h->chunk_rows; }

extern "C" int redio_pfb_os_reserve(redio_pfb_os *h, size_t n_in)
{
    if (!h) return REDIO_ERR_ARG;
    if (redio_pfb_os_route(h) == 1) return REDIO_OK;
    const size_t rows = redio_pfb_os_nrows(h, n_in);
    if (rows == 0) return REDIO_OK;
    const size_t pass = os_pass_rows(h, rows);
    REDIO_TRY(hipSetDevice(h->device));
    if (int rc = scratch_grow(&h->d_v, &h->v_cap, pass * (size_t)h->M, sizeof(float2))) return rc;
    if (h->fft_stages && pass > h->fft_cap) {
        if (int rc = redio_fft_reserve(h->fft, pass)) return rc;
        h->fft_cap = pass;
    }
    return REDIO_OK;
}

extern "C" int redio_pfb_os_enqueue(redio_pfb_os *h, const void *d_in, size_t n_in, uint64_t first_row, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t M = (size_t)h->M, P = (size_t)h->P, H = h->H;
    const size_t rows = redio_pfb_os_nrows(h, n_in);
    if (rows == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return REDIO_ERR_ARG;
    const size_t used = (rows - 1) * H + M * P; // samples the rows read
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + rows * M * sizeof(float2) && o < a + used * sizeof(float2)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const bool fused = (h->flags & REDIO_FIR_FUSED) != 0;
    if (redio_pfb_os_route(h) == 1) {
        const hipError_t e = launch_pfb_os((const float2 *)d_in, h->d_h, redio_fft_twiddles_dev(h->fft), (float2 *)d_out, (long)rows, h->P, first_row, fused, st);
        return e == hipErrorNotSupported ? REDIO_ERR_UNSUPPORTED : hip_rc(e);
    }
    const size_t pass = os_pass_rows(h, rows);
    if (pass * M > h->v_cap || (h->fft_stages && pass > h->fft_cap)) { // un-reserved: grow on first use, never inside a capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = redio_pfb_os_reserve(h, n_in)) return rc;
    }
    // rows [c0, c0 + n) read the samples from c0 H on and nothing of the pass before: passes share input, never scratch
    for (size_t c0 = 0; c0 < rows; c0 += pass) {
        const size_t n = rows - c0 < pass ? rows - c0 : pass;
        const long f0 = (long)((first_row + (uint64_t)c0) % (uint64_t)M); // F + r is taken modulo 2^64
        REDIO_TRY(launch_pfb_os_branch((const float2 *)d_in + c0 * H, h->d_h, (float2 *)h->d_v, (long)n, h->M, h->P, (long)H, f0, fused, st));
        if (int rc = redio_fft_enqueue(h->fft, h->d_v, (float2 *)d_out + c0 * M, n, stream)) return rc;
    }
    return REDIO_OK;
}
