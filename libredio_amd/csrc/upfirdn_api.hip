// upfirdn_api.hip -- the rational resampler's plan (include/redio.h, redio_upfirdn_*): the taps in polyphase order and the per-phase
// table on the device, one launch per call.  The fold is dsputils::convolve's (src/dsputils/src/dsputils.rs:30-32); the contract and the
// phase arithmetic are in upfirdn_core.h, the kernels in upfirdn_kernels.hip, the carried-history form in stream_carry.hip.
#include "../../include/redio.h"
#include "upfirdn_core.h"
#include "redio_internal.h"
#include <new>
#include <vector>

struct redio_upfirdn {
    int device;
    size_t ntaps, up, down;
    size_t Up, Dp, Wp; // one period: outputs, new samples, window
    unsigned flags;
    float *d_taps;                 // sub-filter g_r at d_taps + phase[r].off, each zero-padded to a multiple of 16 floats
    redio::UpfirdnPhase *d_phase;  // Up entries
};

extern "C" int redio_upfirdn_create(redio_upfirdn **h, const float *taps, size_t ntaps, size_t up, size_t down, unsigned flags)
{
    if (!h) return REDIO_ERR_ARG;
    *h = nullptr;
    if (!taps || ntaps == 0 || up == 0 || down == 0) return REDIO_ERR_ARG;
    // down: a window starts s(r) <= down samples in, and the table holds that as an int
    if (ntaps > (size_t)redio::UPFIRDN_MAX_TAPS || up > (size_t)redio::UPFIRDN_MAX_UP || down >= ((size_t)1 << 31)) return REDIO_ERR_UNSUPPORTED;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return REDIO_ERR_NO_DEVICE;
    redio_upfirdn *p = new (std::nothrow) redio_upfirdn();
    if (!p) return REDIO_ERR_NOMEM;
    const long K = (long)ntaps, U = (long)up, D = (long)down;
    p->device = dev; p->ntaps = ntaps; p->up = up; p->down = down; p->flags = flags; p->d_taps = nullptr; p->d_phase = nullptr;
    p->Up = (size_t)redio::upfirdn_period_out(U, D); p->Dp = (size_t)redio::upfirdn_period_in(U, D); p->Wp = (size_t)redio::upfirdn_window(K, U, D);
    std::vector<redio::UpfirdnPhase> ph;
    std::vector<float> tp;
    redio::upfirdn_build(taps, K, U, D, ph, tp);
    hipError_t e = hipMalloc((void **)&p->d_taps, tp.size() * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **)&p->d_phase, ph.size() * sizeof(redio::UpfirdnPhase));
    if (e == hipSuccess) e = hipMemcpy(p->d_taps, tp.data(), tp.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p->d_phase, ph.data(), ph.size() * sizeof(redio::UpfirdnPhase), hipMemcpyHostToDevice);
    if (e != hipSuccess) { redio_upfirdn_destroy(p); return hip_rc(e); }
    *h = p;
    return REDIO_OK;
}
extern "C" int redio_upfirdn_destroy(redio_upfirdn *h)
{
    if (!h) return REDIO_OK;
    if (h->d_taps) hipFree(h->d_taps);
    if (h->d_phase) hipFree(h->d_phase);
    delete h;
    return REDIO_OK;
}
extern "C" size_t redio_upfirdn_nout(const redio_upfirdn *h, size_t n_in)
{
    if (!h || n_in > ((size_t)1 << 46)) return 0; // n_in * up stays far inside 64 bits
    return (size_t)redio::upfirdn_nout(n_in, h->ntaps, h->up, h->down);
}
extern "C" int redio_upfirdn_route(const redio_upfirdn *h) { return h ? redio::upfirdn_route((long)h->ntaps, (long)h->up, (long)h->down) : 0; }
extern "C" size_t redio_upfirdn_period_out(const redio_upfirdn *h) { return h ? h->Up : 0; }
extern "C" size_t redio_upfirdn_period_in(const redio_upfirdn *h) { return h ? h->Dp : 0; }
extern "C" size_t redio_upfirdn_window(const redio_upfirdn *h) { return h ? h->Wp : 0; }

// every argument is checked before anything is launched
static int upfirdn_enqueue(redio_upfirdn *h, const void *d_in, size_t n_in, size_t nout, void *d_out, void *stream)
{
    if (nout == 0) return REDIO_OK;
    if (!d_in || !d_out || d_in == d_out) return REDIO_ERR_ARG;
    const bool cplx = (h->flags & REDIO_FIR_COMPLEX) != 0;
    const size_t el = cplx ? sizeof(float2) : sizeof(float);
    const uintptr_t a = (uintptr_t)d_in, b = (uintptr_t)d_out;
    if (((a | b) & (el - 1)) != 0) return REDIO_ERR_ARG;                       // a whole-sample boundary
    if (a < b + nout * el && b < a + n_in * el) return REDIO_ERR_ARG;          // the ranges overlap
    REDIO_TRY(hipSetDevice(h->device));
    return hip_rc(redio::launch_upfirdn(d_in, (long)n_in, h->d_phase, h->d_taps, (long)h->ntaps, (long)h->up, (long)h->down, d_out, (long)nout, cplx,
                                        (h->flags & REDIO_FIR_FUSED) != 0, (hipStream_t)stream));
}
extern "C" int redio_upfirdn_enqueue(redio_upfirdn *h, const void *d_in, size_t n_in, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    return upfirdn_enqueue(h, d_in, n_in, redio_upfirdn_nout(h, n_in), d_out, stream);
}
// the carried-history layer's entry: exactly `periods` periods (periods * U' outputs), whose windows the n_in samples must hold.  With
// U > D a stateless call on the same samples yields MORE outputs than whole periods, so the stream never goes through the public entry.
int redio_upfirdn_enqueue_periods(redio_upfirdn *h, const void *d_in, size_t n_in, size_t periods, void *d_out, void *stream)
{
    if (!h) return REDIO_ERR_ARG;
    if (periods == 0) return REDIO_OK;
    if (n_in < (periods - 1) * h->Dp + h->Wp) return REDIO_ERR_ARG;
    return upfirdn_enqueue(h, d_in, n_in, periods * h->Up, d_out, stream);
}

void redio_upfirdn_shape(const redio_upfirdn *h, size_t *period_out, size_t *period_in, size_t *window, unsigned *flags, int *device)
{
    *period_out = h->Up; *period_in = h->Dp; *window = h->Wp; *flags = h->flags; *device = h->device;
}
