// fftr_api.hip -- C ABI of the real-input transform plan (include/redio.h, redio_fftr_*): kiss_fftr / kiss_fftri batched on the device.
#include "../../include/redio.h"
#include "fftr_core.h"
#include "redio_internal.h"
#include <new>
#include <vector>

using namespace redio;


struct redio_fftr {
    int device;
    int nfft, M, inverse;
    bool fused;        // N = 2048: one kernel, no scratch
    bool cplx_stages;  // the complex plan of size M stages through a buffer of its own (redio_fft_reserve)
    redio_fft *cplx;   // size M, same direction (none for M = 1: a one-point transform is the identity)
    float2 *d_stw;     // M / 2 super twiddles
    void *d_scratch;   // generic path: nbatch rows of M cf32 between the complex plan and the split pass
    size_t scratch_rows;
};

extern "C" int redio_fftr_create(redio_fftr **h, int nfft, int inverse)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (nfft < 2 || (nfft & 1)) return REDIO_ERR_ARG;
    if (nfft > (1 << 25)) return REDIO_ERR_UNSUPPORTED;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_fftr *p = new (std::nothrow) redio_fftr();
    if (!p) return REDIO_ERR_NOMEM;
    p->device = dev; p->nfft = nfft; p->M = nfft / 2; p->inverse = inverse ? 1 : 0;
    p->fused = nfft == 2 * FFTR1K_M; p->cplx_stages = false; p->cplx = nullptr; p->d_stw = nullptr; p->d_scratch = nullptr; p->scratch_rows = 0;
    int rc = REDIO_OK;
    if (p->M > 1) rc = redio_fft_create(&p->cplx, p->M, p->inverse);
    if (rc == REDIO_OK && p->cplx) p->cplx_stages = redio_fft_stages(p->cplx, false); // never in place: the scratch is on one side
    if (rc == REDIO_OK) {
        std::vector<float2> stw((size_t)(p->M / 2 > 0 ? p->M / 2 : 1), make_float2(0.f, 0.f));
        fftr_super_tw(p->M, p->inverse, stw.data());
        rc = hip_rc(hipMalloc((void **)&p->d_stw, stw.size() * sizeof(float2)));
        if (rc == REDIO_OK) rc = hip_rc(hipMemcpy(p->d_stw, stw.data(), stw.size() * sizeof(float2), hipMemcpyHostToDevice));
    }
    if (rc != REDIO_OK) {
        redio_fftr_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_fftr_destroy(redio_fftr *h)
{
    if (!h) return REDIO_OK;
    redio_fft_destroy(h->cplx);
    if (h->d_stw) hipFree(h->d_stw);
    redio_free(h->d_scratch);
    delete h;
    return REDIO_OK;
}

const float2 *redio_fftr_twiddles_dev(const redio_fftr *h) { return h->cplx ? redio_fft_twiddles_dev(h->cplx) : nullptr; }
const float2 *redio_fftr_super_dev(const redio_fftr *h) { return h->d_stw; }

extern "C" int redio_fftr_is_fused(const redio_fftr *h) { return h && h->fused ? 1 : 0; }

extern "C" int redio_fftr_reserve(redio_fftr *h, size_t nbatch)
{
    if (!h) return REDIO_ERR_ARG;
    if (h->fused || h->M == 1) return REDIO_OK; // no scratch on these paths
    REDIO_TRY(hipSetDevice(h->device));
    if (h->cplx_stages)
        if (int rc = redio_fft_reserve(h->cplx, nbatch)) return rc;
    return scratch_grow(&h->d_scratch, &h->scratch_rows, nbatch, (size_t)h->M * sizeof(float2));
}

extern "C" int redio_fftr_enqueue_strided(redio_fftr *h, const void *d_in, void *d_out, size_t nbatch, long in_stride, long out_stride, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    if (nbatch == 0) return REDIO_OK;
    if (!d_in || !d_out || d_in == d_out) return REDIO_ERR_ARG;
    const int N = h->nfft, M = h->M;
    const long out_row = h->inverse ? N : M + 1;
    const long real_stride = h->inverse ? out_stride : in_stride;
    if (in_stride <= 0 || out_stride < out_row || (real_stride & 1)) return REDIO_ERR_ARG;
    if (((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return REDIO_ERR_ARG; // both sides are read and written as cf32
    hipStream_t st = (hipStream_t)stream;
    REDIO_TRY(hipSetDevice(h->device));
    if (h->fused)
        return hip_rc(launch_fftr1k(h->inverse != 0, d_in, d_out, redio_fft_twiddles_dev(h->cplx), h->d_stw, (long)nbatch, in_stride, out_stride, st));
    if (M == 1) // Z = the row itself
        return hip_rc(launch_fftr_split(h->inverse != 0, (const float2 *)d_in, h->inverse ? in_stride : in_stride / 2, (float2 *)d_out,
                                        h->inverse ? out_stride / 2 : out_stride, h->d_stw, M, (long)nbatch, st));
    if (nbatch > h->scratch_rows) { // grown on first use unless redio_fftr_reserve() sized it; never during graph capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = redio_fftr_reserve(h, nbatch)) return rc;
    }
    float2 *scratch = (float2 *)h->d_scratch;
    if (!h->inverse) {
        if (int rc = redio_fft_enqueue_strided(h->cplx, d_in, scratch, nbatch, in_stride / 2, stream)) return rc;
        return hip_rc(launch_fftr_split(false, scratch, M, (float2 *)d_out, out_stride, h->d_stw, M, (long)nbatch, st));
    }
    REDIO_TRY(launch_fftr_split(true, (const float2 *)d_in, in_stride, scratch, M, h->d_stw, M, (long)nbatch, st));
    if (out_stride == N) return redio_fft_enqueue(h->cplx, scratch, d_out, nbatch, stream);
    for (size_t b = 0; b < nbatch; ++b) // the complex plan writes packed rows: spaced-out rows go one launch each
        if (int rc = redio_fft_enqueue(h->cplx, scratch + b * (size_t)M, (float *)d_out + b * (size_t)out_stride, 1, stream)) return rc;
    return REDIO_OK;
}

extern "C" int redio_fftr_enqueue(redio_fftr *h, const void *d_in, void *d_out, size_t nbatch, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    return redio_fftr_enqueue_strided(h, d_in, d_out, nbatch, h->inverse ? h->M + 1 : h->nfft, h->inverse ? h->nfft : h->M + 1, stream);
}
