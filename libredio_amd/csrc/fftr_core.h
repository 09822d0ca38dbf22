// fftr_core.h -- the real-input transform's split step (kiss_fftr / kiss_fftri, kissfft 1.3.0 tools/kiss_fftr.c as restated in
// DESIGN.md): N real points are M = N / 2 complex points through the complex transform of size M, and one pass that turns
// Z[0 .. M-1] into freq[0 .. M] (forward) or freq[0 .. M] into T[0 .. M-1] (inverse).  Every multiply and add is rounded on its
// own, in the association of the published loop; one step of that loop yields the two elements k and M - k, which is the unit here.
//
// Host-compilable (tests/emu_fftr runs the same thread and lane programs on the CPU).
#pragma once
#include "redio_device.h"
#include <math.h>

namespace redio {

// super_twiddles of kiss_fftr_alloc: M / 2 entries, phase = -pi ((i + 1) / M + 1/2) in double (sign flipped for an inverse cfg),
// each component rounded once.  Host only.
inline void fftr_super_tw(int M, int inverse, float2 *tw)
{
    const double pi = 3.141592653589793238462643383279502884197169399375105820974944;
    for (int i = 0; i < M / 2; ++i) {
        double phase = -pi * ((double)(i + 1) / M + 0.5);
        if (inverse) phase *= -1;
        tw[i] = make_float2((float)cos(phase), (float)sin(phase));
    }
}

// ---- forward: step k of kiss_fftr's loop.  zk = Z[k], zmk = Z[M - k], tw = super_tw[k - 1]; lo = freq[k], hi = freq[M - k]
RD_HD void fftr_fwd_pair(float2 zk, float2 zmk, float2 tw, float2 &lo, float2 &hi)
{
    const float2 fpnk = make_float2(zmk.x, -zmk.y);
    const float2 f1 = cadd_rn(zk, fpnk), f2 = csub_rn(zk, fpnk);
    const float2 w = cmul_rn(f2, tw);
    lo = make_float2(mul_rn(add_rn(f1.x, w.x), 0.5f), mul_rn(add_rn(f1.y, w.y), 0.5f));
    hi = make_float2(mul_rn(sub_rn(f1.x, w.x), 0.5f), mul_rn(sub_rn(w.y, f1.y), 0.5f));
}
// freq[0] and freq[M] from Z[0]
RD_HD void fftr_fwd_ends(float2 z0, float2 &dc, float2 &nyq)
{
    dc = make_float2(add_rn(z0.x, z0.y), 0.f);
    nyq = make_float2(sub_rn(z0.x, z0.y), 0.f);
}

// ---- inverse: step k of kiss_fftri's loop.  fk = freq[k], fmk = freq[M - k], tw = super_tw[k - 1] of the inverse table;
// lo = T[k], hi = T[M - k]
RD_HD void fftr_inv_pair(float2 fk, float2 fmk, float2 tw, float2 &lo, float2 &hi)
{
    const float2 fnkc = make_float2(fmk.x, -fmk.y);
    const float2 fek = cadd_rn(fk, fnkc), tmp = csub_rn(fk, fnkc);
    const float2 fok = cmul_rn(tmp, tw);
    lo = cadd_rn(fek, fok);
    hi = make_float2(sub_rn(fek.x, fok.x), -sub_rn(fek.y, fok.y));
}
// T[0] from freq[0] and freq[M] (their imaginary parts are ignored)
RD_HD float2 fftr_inv_first(float2 f0, float2 fM) { return make_float2(add_rn(f0.x, fM.x), sub_rn(f0.x, fM.x)); }

// ---- any M: thread j = 0 ... M / 2 of one row.  Where 2 j == M both results name element j and the loop's second write wins.
template <typename ZPtr, typename FPtr, typename TwPtr>
RD_HD void fftr_post_thread(int j, int M, ZPtr z, FPtr f, TwPtr stw)
{
    float2 lo, hi;
    if (j == 0) {
        fftr_fwd_ends(z[0], lo, hi);
        f[0] = lo;
        f[M] = hi;
        return;
    }
    fftr_fwd_pair(z[j], z[M - j], stw[j - 1], lo, hi);
    if (2 * j != M) f[j] = lo;
    f[M - j] = hi;
}
template <typename FPtr, typename TPtr, typename TwPtr>
RD_HD void fftr_pre_thread(int j, int M, FPtr f, TPtr t, TwPtr stw)
{
    if (j == 0) {
        t[0] = fftr_inv_first(f[0], f[M]);
        return;
    }
    float2 lo, hi;
    fftr_inv_pair(f[j], f[M - j], stw[j - 1], lo, hi);
    if (2 * j != M) t[j] = lo;
    t[M - j] = hi;
}

// ============================================================================================
// M = 1024 fused into the one-wavefront transform of fft_core.h (fft1k_*): lane L owns the steps k = L + 64 t, t = 0 ... 7
// (k = 0 ... 511; lane 0's t = 0 is the DC / Nyquist pair) and lane 0 also owns k = 512.
//   forward: the transform leaves Z[L + 64 t] in register fftr1k_reg(t) and Z in natural order in the wave's LDS image; the
//            partner Z[1024 - k] comes from LDS (for L != 0 it was lane 64 - L's register fftr1k_reg(15 - t)).
//   inverse: the lane loads freq[k] and freq[1024 - k] from global memory, keeps T[k] as input register t of the transform and
//            hands T[1024 - k] through LDS to the lane and register that feed it (lane 64 - L, register 15 - t; lane 0: register
//            16 - t); input register t of lane L is T[L + 64 t].
// ============================================================================================
constexpr int FFTR1K_M = 1024;
RD_HD int fftr1k_reg(int t) { return 4 * (t & 3) + (t >> 2); } // fft1k_wave_regs leaves X[lane + 64 q + 256 j] in v[4 q + j]
RD_HD int fftr1k_partner(int lane, int t) { return FFTR1K_M - (lane + 64 * t); } // 1024 (lane 0, t 0) stands for the Nyquist slot

struct Fftr1kTw {
    float2 s[8]; // super_tw[lane + 64 t - 1]
    float2 mid;  // super_tw[511], the step k = 512
};
template <typename TwPtr>
RD_HD void fftr1k_load_tw(Fftr1kTw &w, int lane, TwPtr stw)
{
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = lane + 64 * t;
        w.s[t] = stw[k > 0 ? k - 1 : 0]; // lane 0, t = 0: not used
    }
    w.mid = stw[FFTR1K_M / 2 - 1];
}

// forward split by lane `lane`: v = the transform's result registers, ex = Z in natural order (LDS), f = the row's M + 1 outputs
template <typename ExPtr, typename FPtr>
RD_HD void fftr1k_post_lane(const float2 (&v)[16], ExPtr ex, const Fftr1kTw &w, int lane, FPtr f)
{
    float2 lo, hi;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int k = lane + 64 * t;
        const float2 zk = v[fftr1k_reg(t)];
        if (t == 0 && lane == 0) {
            fftr_fwd_ends(zk, lo, hi);
        } else {
            const float2 zm = ex[fftr1k_partner(lane, t)];
            fftr_fwd_pair(zk, zm, w.s[t], lo, hi);
        }
        f[k] = lo;
        f[FFTR1K_M - k] = hi;
    }
    if (lane == 0) {
        const float2 z = v[fftr1k_reg(8)];
        fftr_fwd_pair(z, z, w.mid, lo, hi);
        f[FFTR1K_M / 2] = hi;
    }
}

// the same split with its results kept in registers, in the layout fftr1k_load_row() produces: a[t] = freq[k], b[t] = freq[1024 - k]
// (k = lane + 64 t), mid = freq[512] (lane 0; the other lanes never use theirs).  For a consumer that goes on to the inverse split in
// the same wave (ovsave_real_kernels.hip).
template <typename ExPtr>
RD_HD void fftr1k_post_lane_regs(const float2 (&v)[16], ExPtr ex, const Fftr1kTw &w, int lane, float2 (&a)[8], float2 (&b)[8], float2 &mid)
{
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const float2 zk = v[fftr1k_reg(t)];
        if (t == 0 && lane == 0) {
            fftr_fwd_ends(zk, a[0], b[0]);
        } else {
            const float2 zm = ex[fftr1k_partner(lane, t)];
            fftr_fwd_pair(zk, zm, w.s[t], a[t], b[t]);
        }
    }
    mid = make_float2(0.f, 0.f);
    if (lane == 0) {
        float2 lo;
        const float2 z = v[fftr1k_reg(8)];
        fftr_fwd_pair(z, z, w.mid, lo, mid);
    }
}

// the inverse's loads of one row by lane `lane`: a[t] = freq[k], b[t] = freq[1024 - k] (k = lane + 64 t), mid = freq[512]
template <typename FPtr>
RD_HD void fftr1k_load_row(FPtr f, int lane, float2 (&a)[8], float2 (&b)[8], float2 &mid)
{
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        a[t] = f[lane + 64 * t];
        b[t] = f[fftr1k_partner(lane, t)];
    }
    mid = f[FFTR1K_M / 2];
}

// inverse split by lane `lane`: a[t] = freq[k], b[t] = freq[1024 - k] (k = lane + 64 t), mid = freq[512]; writes the input registers
// v[0 .. 7] and the LDS slots 512 ... 1023 of T.  After a wave_lds_fence() fftr1k_pre_gather() fills v[8 .. 15].
template <typename ExPtr>
RD_HD void fftr1k_pre_lane(const float2 (&a)[8], const float2 (&b)[8], float2 mid, const Fftr1kTw &w, int lane, float2 (&v)[16], ExPtr ex)
{
    float2 lo, hi;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t == 0 && lane == 0) {
            v[0] = fftr_inv_first(a[0], b[0]);
        } else {
            fftr_inv_pair(a[t], b[t], w.s[t], lo, hi);
            v[t] = lo;
            ex[fftr1k_partner(lane, t)] = hi;
        }
    }
    if (lane == 0) {
        fftr_inv_pair(mid, mid, w.mid, lo, hi);
        ex[FFTR1K_M / 2] = hi;
    }
}
template <typename ExPtr>
RD_HD void fftr1k_pre_gather(float2 (&v)[16], ExPtr ex, int lane)
{
#pragma unroll
    for (int t = 8; t < 16; ++t) v[t] = ex[lane + 64 * t];
}

} // namespace redio
