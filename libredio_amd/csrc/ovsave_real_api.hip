// ovsave_real_api.hip -- C ABI of overlap-save on real streams (include/redio.h, redio_ovsave_real_*): the valid-mode correlation of
// dsputils::convolve (src/dsputils/src/dsputils.rs:30-32) on f32 samples with real taps, evaluated per block of N = nfft samples
// with the real-input transforms kiss_fftr / kiss_fftri (fftr_core.h):
//     X = kiss_fftr(block b at x + b*hop),  Y = X .* Hc,  y = kiss_fftri(Y),  out[b*hop + i] = y[i] * (1/N), i < hop
// with Ke = ntaps | 1, hop = N - Ke + 1 (always even) and Hc = conj(kiss_fftr(taps zero-padded to N)).
// Algorithmic bytes per output sample: 4 N / hop read + 4 written -- half of what redio_ovsave_* moves for a widened stream.
//   N = 2048     one kernel, nothing but registers and one LDS image per wave (ovsave_real_kernels.hip)
//   other N      forward redio_fftr with in_stride = hop -> product -> inverse redio_fftr -> scaled copy, through plan-owned
//                scratch, in chunks of blocks
#include "../../include/redio.h"
#include "redio_internal.h"
#include <new>
#include <vector>

using namespace redio;


struct redio_ovsave_real {
    int device, nfft;
    size_t ntaps, hop;
    bool fused;            // N = 2048: one kernel, no scratch
    redio_fftr *fw, *bw;   // kiss_fftr / kiss_fftri of N points
    float2 *d_Hc;          // N / 2 + 1 bins
    size_t chunk_blocks;   // generic path: blocks per pass through the scratch
    void *d_spec, *d_rows; // generic path: scratch_rows rows of N / 2 + 1 cf32, and of N f32
    size_t scratch_rows;
};

extern "C" int redio_ovsave_real_create(redio_ovsave_real **h, const float *taps, size_t ntaps, int nfft)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!taps || nfft < 2 || (nfft & 1)) return REDIO_ERR_ARG;
    if (ntaps == 0 || (ntaps | 1) > (size_t)nfft) return REDIO_ERR_ARG;
    if (nfft > (1 << 25)) return REDIO_ERR_UNSUPPORTED; // redio_fftr_create's ceiling
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_ovsave_real *p = new (std::nothrow) redio_ovsave_real();
    if (!p) return REDIO_ERR_NOMEM;
    p->device = dev; p->nfft = nfft; p->ntaps = ntaps; p->hop = (size_t)nfft - (ntaps | 1) + 1;
    p->fused = nfft == 2048;
    p->fw = p->bw = nullptr; p->d_Hc = nullptr; p->d_spec = p->d_rows = nullptr; p->scratch_rows = 0;
    // 64 MiB of real rows per chunk (the complex operator's work-buffer size, ovsave.hip), at least one block
    p->chunk_blocks = ((size_t)64 << 20) / ((size_t)nfft * sizeof(float));
    if (p->chunk_blocks < 1) p->chunk_blocks = 1;
    const int nbins = nfft / 2 + 1;
    int rc = redio_fftr_create(&p->fw, nfft, 0);
    if (rc == REDIO_OK) rc = redio_fftr_create(&p->bw, nfft, 1);
    if (rc == REDIO_OK) rc = hip_rc(hipMalloc((void **)&p->d_Hc, (size_t)nbins * sizeof(float2)));
    if (rc == REDIO_OK) { // H by the plan's own forward transform of the padded taps, then the conjugate
        float *d_pad = nullptr;
        rc = hip_rc(hipMalloc((void **)&d_pad, (size_t)nfft * sizeof(float)));
        if (rc == REDIO_OK) {
            std::vector<float> hp((size_t)nfft, 0.f);
            for (size_t j = 0; j < ntaps; ++j) hp[j] = taps[j];
            rc = hip_rc(hipMemcpy(d_pad, hp.data(), (size_t)nfft * sizeof(float), hipMemcpyHostToDevice));
        }
        if (rc == REDIO_OK) rc = redio_fftr_enqueue(p->fw, d_pad, p->d_Hc, 1, nullptr);
        if (rc == REDIO_OK) rc = hip_rc(launch_ovsave_real_conj(p->d_Hc, nbins, nullptr));
        if (rc == REDIO_OK) rc = hip_rc(hipDeviceSynchronize());
        if (d_pad) hipFree(d_pad);
    }
    if (rc != REDIO_OK) {
        redio_ovsave_real_destroy(p);
        return rc;
    }
    *h = p;
    return REDIO_OK;
}

extern "C" int redio_ovsave_real_destroy(redio_ovsave_real *h)
{
    if (!h) return REDIO_OK;
    redio_fftr_destroy(h->fw); redio_fftr_destroy(h->bw);
    if (h->d_Hc) hipFree(h->d_Hc);
    redio_free(h->d_spec); redio_free(h->d_rows);
    delete h;
    return REDIO_OK;
}

void redio_ovsave_real_shape(const redio_ovsave_real *h, int *nfft, size_t *hop, int *device) { *nfft = h->nfft; *hop = h->hop; *device = h->device; }

extern "C" size_t redio_ovsave_real_nout(const redio_ovsave_real *h, size_t n_in)
{
    if (!h || n_in < (size_t)h->nfft) return 0;
    return ((n_in - (size_t)h->nfft) / h->hop + 1) * h->hop;
}

extern "C" int redio_ovsave_real_is_fused(const redio_ovsave_real *h) { return h && h->fused ? 1 : 0; }

extern "C" int redio_ovsave_real_reserve(redio_ovsave_real *h, size_t n_in)
{
    if (!h) return REDIO_ERR_ARG;
    if (h->fused) return REDIO_OK; // no scratch on this path
    size_t rows = redio_ovsave_real_nout(h, n_in) / h->hop;
    if (rows > h->chunk_blocks) rows = h->chunk_blocks;
    if (rows <= h->scratch_rows) return REDIO_OK;
    REDIO_TRY(hipSetDevice(h->device));
    if (int rc = redio_fftr_reserve(h->fw, rows)) return rc;
    if (int rc = redio_fftr_reserve(h->bw, rows)) return rc;
    size_t spec_rows = h->scratch_rows, rows_rows = h->scratch_rows; // one capacity for both buffers: it counts only once both have grown
    h->scratch_rows = 0;
    if (int rc = scratch_grow(&h->d_spec, &spec_rows, rows, (size_t)(h->nfft / 2 + 1) * sizeof(float2))) return rc;
    if (int rc = scratch_grow(&h->d_rows, &rows_rows, rows, (size_t)h->nfft * sizeof(float))) return rc;
    h->scratch_rows = rows;
    return REDIO_OK;
}

int redio_ovsave_real_enqueue_any(redio_ovsave_real *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    const size_t nout = redio_ovsave_real_nout(h, n_in);
    if (nout == 0) return REDIO_OK;
    if (!d_in || !d_out || d_in == d_out) return REDIO_ERR_ARG;
    if (((uintptr_t)d_in & 3) || ((uintptr_t)d_out & 7)) return REDIO_ERR_ARG;
    REDIO_TRY(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t nblk = nout / h->hop;
    const float scale = 1.0f / (float)h->nfft;
    const float *x = (const float *)d_in;
    float *out = (float *)d_out;
    if (h->fused)
        return hip_rc(launch_ovsave_real2k(x, (long)h->hop, redio_fftr_twiddles_dev(h->fw), redio_fftr_twiddles_dev(h->bw), redio_fftr_super_dev(h->fw),
                                           redio_fftr_super_dev(h->bw), h->d_Hc, out, (long)nblk, scale, st));
    const size_t need = nblk < h->chunk_blocks ? nblk : h->chunk_blocks;
    if (need > h->scratch_rows) { // grown on first use unless redio_ovsave_real_reserve() sized it; never during graph capture
        if (stream_capturing(st)) return REDIO_ERR_NOT_RESERVED;
        if (int rc = redio_ovsave_real_reserve(h, n_in)) return rc;
    }
    const long N = h->nfft, nbins = N / 2 + 1;
    const bool aligned = ((uintptr_t)d_in & 7) == 0;
    for (size_t b0 = 0; b0 < nblk; b0 += h->chunk_blocks) {
        const size_t nb = (nblk - b0 < h->chunk_blocks) ? nblk - b0 : h->chunk_blocks;
        const float *xb = x + b0 * h->hop;
        if (aligned) {
            if (int rc = redio_fftr_enqueue_strided(h->fw, xb, h->d_spec, nb, (long)h->hop, nbins, stream)) return rc;
        } else { // the transform reads pairs: pack the blocks into the real scratch first
            REDIO_TRY(launch_ovsave_real_rows(xb, (float *)h->d_rows, (long)nb, N, (long)h->hop, st));
            if (int rc = redio_fftr_enqueue_strided(h->fw, h->d_rows, h->d_spec, nb, N, nbins, stream)) return rc;
        }
        REDIO_TRY(launch_ovsave_real_mul((float2 *)h->d_spec, h->d_Hc, (long)nb, (int)nbins, st));
        if (int rc = redio_fftr_enqueue_strided(h->bw, h->d_spec, h->d_rows, nb, nbins, N, stream)) return rc;
        REDIO_TRY(launch_ovsave_real_scale_out((const float *)h->d_rows, out + b0 * h->hop, (long)nb, N, (long)h->hop, scale, st));
    }
    return REDIO_OK;
}

extern "C" int redio_ovsave_real_enqueue(redio_ovsave_real *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    if (redio_ovsave_real_nout(h, n_in) == 0) return REDIO_OK;
    if (!d_in || !d_out || ((uintptr_t)d_in & 7) || ((uintptr_t)d_out & 7)) return REDIO_ERR_ARG;
    const char *a = (const char *)d_in, *o = (const char *)d_out; // the ranges read and written must not overlap
    if (a < o + redio_ovsave_real_nout(h, n_in) * sizeof(float) && o < a + n_in * sizeof(float)) return REDIO_ERR_ARG;
    return redio_ovsave_real_enqueue_any(h, d_in, n_in, d_out, stream);
}
