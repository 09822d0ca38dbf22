// ddc_upfirdn_api.hip -- the tuned resampler's plan (include/redio.h, redio_ddc_upfirdn_*): the tuner's oscillator table, the resampler's
// polyphase taps and per-phase table on the device, one launch per call.  kpn::mul_vecs (src/kpn/src/kpn.rs:198-203) by the table, then
// the polyphase form of dsputils::convolve (src/dsputils/src/dsputils.rs:30-32); the contract is in ddc_upfirdn_core.h, the kernels in
// ddc_upfirdn_kernels.hip, the carried-history form in stream_carry.hip.
#include "../../include/redio.h"
#include "ddc_upfirdn_core.h"
#include "redio_internal.h"
#include <new>
#include <vector>

struct redio_ddc_upfirdn {
    int device;
    size_t ntaps, up, down, period;
    size_t Up, Dp, Wp; // one period of the resampler: outputs, new samples, window
    unsigned flags;
    float *d_taps;                 // sub-filter g_r at d_taps + phase[r].off, each zero-padded to a multiple of 16 floats (upfirdn_build)
    redio::UpfirdnPhase *d_phase;  // Up entries
    float2 *d_tab;                 // period + DDC_TABLE_EXT entries: entry e = osc[e mod period] (ddc_core.h)
};

extern "C" int redio_ddc_upfirdn_create(redio_ddc_upfirdn **h, const float *osc, size_t period, const float *taps, size_t ntaps, size_t up, size_t down,
                                        unsigned flags)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!osc || !taps || period == 0 || period > REDIO_DDC_MAX_PERIOD || ntaps == 0 || up == 0 || down == 0) return REDIO_ERR_ARG;
    // down: a window starts s(r) <= down samples in, and the table holds that as an int
    if (ntaps > (size_t)redio::UPFIRDN_MAX_TAPS || up > (size_t)redio::UPFIRDN_MAX_UP || down >= ((size_t)1 << 31)) return REDIO_ERR_UNSUPPORTED;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_ddc_upfirdn *p = new (std::nothrow) redio_ddc_upfirdn();
    if (!p) return REDIO_ERR_NOMEM;
    const long K = (long)ntaps, U = (long)up, D = (long)down;
    p->device = dev; p->ntaps = ntaps; p->up = up; p->down = down; p->period = period; p->flags = flags;
    p->d_taps = nullptr; p->d_phase = nullptr; p->d_tab = nullptr;
    p->Up = (size_t)redio::upfirdn_period_out(U, D); p->Dp = (size_t)redio::upfirdn_period_in(U, D); p->Wp = (size_t)redio::upfirdn_window(K, U, D);
    std::vector<redio::UpfirdnPhase> ph;
    std::vector<float> tp;
    redio::upfirdn_build(taps, K, U, D, ph, tp);
    const size_t ntab = period + (size_t)redio::DDC_TABLE_EXT;
    std::vector<float> tb(2 * ntab);
    for (size_t e = 0; e < ntab; ++e) memcpy(&tb[2 * e], &osc[2 * (e % period)], 2 * sizeof(float));
    hipError_t e = hipMalloc((void **)&p->d_taps, tp.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_phase, ph.size() * sizeof(redio::UpfirdnPhase));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_tab, ntab * sizeof(float2));
    if (e == hipSuccess) e = hipMemcpy(p->d_taps, tp.data(), tp.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_phase, ph.data(), ph.size() * sizeof(redio::UpfirdnPhase), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_tab, tb.data(), ntab * sizeof(float2), hipMemcpyHostToDevice);
    if (e != hipSuccess) { redio_ddc_upfirdn_destroy(p); return hip_rc(e); }
    *h = p;
    return REDIO_OK;
}
extern "C" int redio_ddc_upfirdn_destroy(redio_ddc_upfirdn *h)
{
    if (!h) return REDIO_OK;
    if (h->d_taps) hipFree(h->d_taps);
    if (h->d_phase) hipFree(h->d_phase);
    if (h->d_tab) hipFree(h->d_tab);
    delete h;
    return REDIO_OK;
}
extern "C" size_t redio_ddc_upfirdn_nout(const redio_ddc_upfirdn *h, size_t n_in)
{
    if (!h || n_in > ((size_t)1 << 46)) return 0; // redio_upfirdn_nout: n_in * up stays far inside 64 bits
    return (size_t)redio::upfirdn_nout(n_in, h->ntaps, h->up, h->down);
}
// the route is the resampler's on the cf32 geometry: the output is always cf32, and upfirdn_r decides on cf32 elements
extern "C" int redio_ddc_upfirdn_route(const redio_ddc_upfirdn *h) { return h ? redio::upfirdn_route((long)h->ntaps, (long)h->up, (long)h->down) : 0; }
extern "C" size_t redio_ddc_upfirdn_period(const redio_ddc_upfirdn *h) { return h ? h->period : 0; }
extern "C" size_t redio_ddc_upfirdn_period_out(const redio_ddc_upfirdn *h) { return h ? h->Up : 0; }
extern "C" size_t redio_ddc_upfirdn_period_in(const redio_ddc_upfirdn *h) { return h ? h->Dp : 0; }
extern "C" size_t redio_ddc_upfirdn_window(const redio_ddc_upfirdn *h) { return h ? h->Wp : 0; }

// every argument is checked before anything is launched.  in_elem: bytes per input sample, 8 (cf32) or 2 (u8 I/Q)
static int ddc_upfirdn_enqueue(redio_ddc_upfirdn *h, const void *d_in, size_t n_in, size_t in_elem, size_t nout, uint64_t first_index, void *d_out,
                               void *stream)
{
    if (nout == 0) return REDIO_OK;
    if (!d_in || !d_out || d_in == d_out) return REDIO_ERR_ARG;
    const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out;
    if ((b & 7) != 0 || (in_elem == 8 && (a & 7) != 0)) return REDIO_ERR_ARG;          // cf32 on a whole-sample boundary; bytes anywhere
    if (a < b + nout * sizeof(float2) && b < a + n_in * in_elem) return REDIO_ERR_ARG; // the ranges overlap
    REDIO_TRY(hipSetDevice(h->device));
    return hip_rc(redio::launch_ddc_upfirdn(d_in, in_elem == 2, (long)n_in, redio::ddc_first_mod(first_index, (unsigned)h->period), h->d_tab,
                                            (unsigned)h->period, h->d_phase, h->d_taps, (long)h->ntaps, (long)h->up, (long)h->down, (float2 *)d_out,
                                            (long)nout, (h->flags & REDIO_FIR_FUSED) != 0, (hipStream_t)stream));
}
extern "C" int redio_ddc_upfirdn_enqueue(redio_ddc_upfirdn *h, const void *d_in, size_t n_in, uint64_t first_index, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    return ddc_upfirdn_enqueue(h, d_in, n_in, sizeof(float2), redio_ddc_upfirdn_nout(h, n_in), first_index, d_out, stream);
}
extern "C" int redio_ddc_upfirdn_enqueue_u8(redio_ddc_upfirdn *h, const void *d_bytes, size_t nbytes, uint64_t first_index, void *d_out, void *stream)
{
    if (!h || (nbytes & 1)) return REDIO_ERR_ARG;
    return ddc_upfirdn_enqueue(h, d_bytes, nbytes / 2, 2, redio_ddc_upfirdn_nout(h, nbytes / 2), first_index, d_out, stream);
}
// the carried-history layer's entry: exactly `periods` periods (periods * U' outputs), whose windows the n_in samples must hold.  With
// U > D a stateless call on the same samples yields MORE outputs than whole periods, so the stream never goes through the public entries.
int redio_ddc_upfirdn_enqueue_periods(redio_ddc_upfirdn *h, const void *d_in, size_t n_in, bool u8, size_t periods, uint64_t first_index, void *d_out,
                                      void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    if (periods == 0) return REDIO_OK;
    if (n_in < (periods - 1) * h->Dp + h->Wp) return REDIO_ERR_ARG;
    return ddc_upfirdn_enqueue(h, d_in, n_in, u8 ? 2 : sizeof(float2), periods * h->Up, first_index, d_out, stream);
}

void redio_ddc_upfirdn_shape(const redio_ddc_upfirdn *h, size_t *period_out, size_t *period_in, size_t *window, int *device)
{
    *period_out = h->Up; *period_in = h->Dp; *window = h->Wp; *device = h->device;
}
