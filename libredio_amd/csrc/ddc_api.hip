// ddc_api.hip -- the tuner's plan (include/redio.h, redio_ddc_*): a periodic oscillator table and FIR taps on the device, one launch per
// call.  kpn::mul_vecs (src/kpn/src/kpn.rs:198-203) by the table, then dsputils::convolve (src/dsputils/src/dsputils.rs:30-32); the
// kernels are in ddc_kernels.hip, the carried-history form in stream_carry.hip.
#include "../../include/redio.h"
#include "ddc_core.h"
#include "redio_internal.h"
#include <new>
#include <vector>

struct redio_ddc {
    int device;
    size_t ntaps, decim, period;
    unsigned flags;
    float *d_taps;   // padded to a multiple of 16 floats, as redio_fir's
    float2 *d_tab;   // period + DDC_TABLE_EXT entries: entry e = osc[e mod period] (ddc_core.h)
};

extern "C" int redio_ddc_create(redio_ddc **h, const float *osc, size_t period, const float *taps, size_t ntaps, size_t decim, unsigned flags)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!osc || !taps || period == 0 || period > REDIO_DDC_MAX_PERIOD || ntaps == 0 || decim == 0) return REDIO_ERR_ARG;
    if (ntaps > (1u << 24)) return REDIO_ERR_UNSUPPORTED;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_ddc *p = new (std::nothrow) redio_ddc();
    if (!p) return REDIO_ERR_NOMEM;
    p->device = dev; p->ntaps = ntaps; p->decim = decim; p->period = period; p->flags = flags; p->d_taps = nullptr; p->d_tab = nullptr;
    const size_t padded = (ntaps + 15) & ~(size_t)15, ntab = period + (size_t)redio::DDC_TABLE_EXT;
    std::vector<float> tp(padded, 0.0f), tb(2 * ntab);
    memcpy(tp.data(), taps, ntaps * sizeof(float));
    for (size_t e = 0; e < ntab; ++e) memcpy(&tb[2 * e], &osc[2 * (e % period)], 2 * sizeof(float));
    hipError_t e = hipMalloc((void **)&p->d_taps, padded * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_tab, ntab * sizeof(float2));
    if (e == hipSuccess) e = hipMemcpy(p->d_taps, tp.data(), padded * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_tab, tb.data(), ntab * sizeof(float2), hipMemcpyHostToDevice);
    if (e != hipSuccess) { redio_ddc_destroy(p); return hip_rc(e); }
    *h = p;
    return REDIO_OK;
}
extern "C" int redio_ddc_destroy(redio_ddc *h)
{
    if (!h) return REDIO_OK;
    if (h->d_taps) hipFree(h->d_taps);
    if (h->d_tab) hipFree(h->d_tab);
    delete h;
    return REDIO_OK;
}
extern "C" size_t redio_ddc_nout(const redio_ddc *h, size_t n_in)
{
    if (!h || n_in < h->ntaps) return 0;
    return (n_in - h->ntaps) / h->decim + 1; // redio_fir_nout
}
extern "C" size_t redio_ddc_period(const redio_ddc *h) { return h ? h->period : 0; }
extern "C" int redio_ddc_route(const redio_ddc *h) { return h ? redio::ddc_route((long)h->ntaps, (long)h->decim) : 0; }

static int ddc_enqueue(redio_ddc *h, const void *d_in, size_t n_in, size_t in_elem, uint64_t first_index, void *d_out, void *stream)
{
    const size_t nout = redio_ddc_nout(h, n_in);
    if (nout == 0) return REDIO_OK;
    if (!d_in || !d_out || d_in == d_out) return REDIO_ERR_ARG;
    const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out;
    if (a < b + nout * sizeof(float2) && b < a + n_in * in_elem) return REDIO_ERR_ARG; // the ranges overlap
    REDIO_TRY(hipSetDevice(h->device));
    return hip_rc(redio::launch_ddc(d_in, in_elem == 2, (long)n_in, redio::ddc_first_mod(first_index, (unsigned)h->period), h->d_tab, (unsigned)h->period,
                                    h->d_taps, (int)h->ntaps, (long)h->decim, (float2 *)d_out, (long)nout, (h->flags & REDIO_FIR_FUSED) != 0,
                                    (hipStream_t)stream));
}
extern "C" int redio_ddc_enqueue(redio_ddc *h, const void *d_in, size_t n_in, uint64_t first_index, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    return ddc_enqueue(h, d_in, n_in, sizeof(float2), first_index, d_out, stream);
}
extern "C" int redio_ddc_enqueue_u8(redio_ddc *h, const void *d_bytes, size_t nbytes, uint64_t first_index, void *d_out, void *stream)
{
    if (!h || (nbytes & 1)) return REDIO_ERR_ARG;
    return ddc_enqueue(h, d_bytes, nbytes / 2, 2, first_index, d_out, stream);
}

void redio_ddc_shape(const redio_ddc *h, size_t *ntaps, size_t *decim, int *device)
{
    *ntaps = h->ntaps; *decim = h->decim; *device = h->device;
}
