// ddc_core.h -- the tuner's tile loader: oscillator mix fused into the FIR tile load (include/redio.h, redio_ddc_*).
//
// Arithmetic contract: kpn::mul_vecs (src/kpn/src/kpn.rs:198-203) with a periodic constant vector, then dsputils::convolve
// (src/dsputils/src/dsputils.rs:30-32):
//   m[n] = cmul_rn(x[n], w[(first + n) mod L])     every operation rounded on its own, never contracted
//   y[i] = the FIR fold over m[i*D + j] * h[j]     (fir_core.h: strict tap order; FUSED selects fmaf for the fold only)
// The loader writes m into the SAME padded LDS image the FIR kernels stage (fir_tile.h), so the FIR's two tiled kernel bodies
// (fir_tile_kernels.h) run with it as their loader policy (DdcTile below) and nothing else changed.  The u8 entry converts each byte with i2f (redio_device.h: the arithmetic of redio_data_to_samples) first.
//
// Table index.  The device table holds the period's L entries and then repeats them for DDC_TABLE_EXT more (entry e = w[e mod L]).
// A workgroup takes ONE 64-bit modulo, base = (first + in0) mod L for its tile's first sample in0; a lane then reads entry
// base + n for tile sample n < tile_in + 2 <= DDC_TABLE_EXT -- consecutive addresses, so two entries are one 16-byte load when base
// is even (two 8-byte loads when it is odd), and no lane pays a modulo (an unsigned 32-bit remainder by a run-time L is some twenty
// vector instructions per sample on gfx950, against the eight of the mix itself).  The cost is DDC_TABLE_EXT * 8 = 160 KiB of table
// per plan, L2-resident.  Samples beyond n_in are written as zeros without a table read, and base + n stays inside the allocation
// for every n a loader thread can form.  The direct kernel (no tile) takes one modulo per thread and wraps by compare.
//
// Host-compilable (tests/emu_ddc runs every thread of a workgroup's loader on the CPU).
#pragma once
#include "fir_core.h"
#include "fir_tile.h"

namespace redio {

constexpr unsigned DDC_MAX_PERIOD = 65536;   // REDIO_DDC_MAX_PERIOD
constexpr int DDC_TABLE_EXT = 20480;         // entries behind the period: above the longest tile any route stages (150 KiB of cf32 + 2)

RD_HD unsigned ddc_first_mod(unsigned long long first, unsigned L) { return (unsigned)(first % L); }
// table entry of tile sample 0: (first + in0) mod L from first mod L, without overflow for any first
RD_HD unsigned ddc_base(unsigned first_mod, unsigned long long in0, unsigned L) { return (unsigned)(((unsigned long long)first_mod + in0 % L) % L); }

// The any-taps chunked route's shape under the tuner's names: the shared table and tile of fir_tile.h, nothing of its own
RD_HD constexpr int ddc_chunked_r(long D) { return tile_r(D); } // 0: no chunked form
RD_HD constexpr int ddc_chunked_chw(long D) { return tile_chw(D); }
RD_HD constexpr long ddc_chunked_tile_in(int K, long D, int R) { return tile_in(R, D, tile_window(K)); }
RD_HD constexpr long ddc_chunked_lds_elems(int K, long D, int R) { return tile_lds_elems(R, D, tile_window(K)); }
constexpr long DDC_CHUNKED_LDS_MAX = TILE_LDS_MAX; // bytes: beyond it the direct kernel runs
// redio_ddc_route: 1 specialised tiled (127 and 63 taps at /5 and /1), 2 any-taps chunked, 3 direct
RD_HD constexpr int ddc_route(long K, long D)
{
    if ((K == 127 || K == 63) && (D == 5 || D == 1)) return 1;
    if (K <= (1 << 20) && ddc_chunked_r(D) && ddc_chunked_lds_elems((int)K, D, ddc_chunked_r(D)) * 8 <= DDC_CHUNKED_LDS_MAX) return 2;
    return 3;
}

// one u8 I/Q sample (rtlsdr.rs:159-162), mixed
RD_HD float2 ddc_mix_u8(unsigned bi, unsigned bq, float2 w) { return cmul_rn(make_float2(i2f(bi), i2f(bq)), w); }

// two consecutive table entries from tab + n (n even): one 16-byte load when the workgroup's base is even
RD_HD void ddc_tab2(const float2 *tab, int n, bool tab_vec, float2 &w0, float2 &w1)
{
    if (tab_vec) {
        const float4 q = *reinterpret_cast<const float4 *>(tab + n);
        w0 = make_float2(q.x, q.y); w1 = make_float2(q.z, q.w);
    } else {
        w0 = tab[n]; w1 = tab[n + 1];
    }
}

// The loader of ONE thread `tid` of NT.  x: the tile's first sample (cf32, or with U8 its first byte: two bytes per sample); left:
// samples of the stream from there on (n_in - in0, >= 1); tab: table + base; tile_in: samples the tile holds; put(n, v) writes tile
// sample n into the image.  vec_x: x is 16-byte (cf32) or 4-byte (u8) aligned -- two samples per load; tab_vec: tab is 16-byte aligned.
// STREAM: non-temporal input loads (the FIR kernels' per-shape policy); the table never gets them.
template <bool U8, bool STREAM, typename Put>
RD_HD void ddc_load_thread(int tid, int NT, const void *x, long left, const float2 *tab, int tile_in, bool vec_x, bool tab_vec, Put &&put)
{
    const float2 *xc = reinterpret_cast<const float2 *>(x);
    const unsigned char *xb = reinterpret_cast<const unsigned char *>(x);
    auto one = [&](int n) { // the scalar path of sample n
        float2 m = make_float2(0.f, 0.f);
        if (n < left) {
            if constexpr (U8) m = ddc_mix_u8(xb[2 * n], xb[2 * n + 1], tab[n]);
            else m = cmul_rn(xc[n], tab[n]);
        }
        put(n, m);
    };
    if (vec_x) {
        const int nv = (tile_in + 1) / 2;
        int vfirst = tid;
        if (2L * nv <= left) {
            // the whole tile exists (workgroup-uniform): LB sample loads and LB table loads in flight per lane, no bound checks, for
            // as long as all LB exist; the guarded loop below takes what is left
            constexpr int LB = U8 ? 2 : 4; // u8: four in flight cost ddc_tiled_kernel<63, 5> from bytes its eighth wave per SIMD (65 VGPRs)
            for (; vfirst + (LB - 1) * NT < nv; vfirst += LB * NT) {
                float4 q[LB];   // cf32: two samples
                unsigned u[LB]; // u8: their four bytes, converted behind the loads
                float2 w0[LB], w1[LB];
#pragma unroll
                for (int b = 0; b < LB; ++b) {
                    const int v = vfirst + b * NT;
                    if constexpr (U8) u[b] = reinterpret_cast<const unsigned *>(xb)[v];
                    else q[b] = tile_ld16<STREAM>(reinterpret_cast<const float4 *>(xc) + v);
                }
#pragma unroll
                for (int b = 0; b < LB; ++b) ddc_tab2(tab, 2 * (vfirst + b * NT), tab_vec, w0[b], w1[b]);
#pragma unroll
                for (int b = 0; b < LB; ++b) {
                    const int n = 2 * (vfirst + b * NT);
                    if constexpr (U8) q[b] = make_float4(i2f(u[b] & 255u), i2f((u[b] >> 8) & 255u), i2f((u[b] >> 16) & 255u), i2f(u[b] >> 24));
                    put(n, cmul_rn(make_float2(q[b].x, q[b].y), w0[b]));
                    if (n + 1 < tile_in) put(n + 1, cmul_rn(make_float2(q[b].z, q[b].w), w1[b]));
                }
            }
        }
#pragma unroll 4
        for (int v = vfirst; v < nv; v += NT) {
            const int n = 2 * v;
            if (n + 2 <= left) {
                float2 x0, x1, w0, w1;
                if constexpr (U8) {
                    const unsigned q = reinterpret_cast<const unsigned *>(xb)[v]; // the four bytes of two samples
                    x0 = make_float2(i2f(q & 255u), i2f((q >> 8) & 255u));
                    x1 = make_float2(i2f((q >> 16) & 255u), i2f(q >> 24));
                } else {
                    const float4 q = tile_ld16<STREAM>(reinterpret_cast<const float4 *>(xc) + v);
                    x0 = make_float2(q.x, q.y); x1 = make_float2(q.z, q.w);
                }
                ddc_tab2(tab, n, tab_vec, w0, w1);
                put(n, cmul_rn(x0, w0));
                if (n + 1 < tile_in) put(n + 1, cmul_rn(x1, w1));
            } else {
                one(n);
                if (n + 1 < tile_in) one(n + 1);
            }
        }
    } else {
#pragma unroll 4
        for (int n = tid; n < tile_in; n += NT) one(n);
    }
}

// The loader as the policy of the FIR's two tiled kernel bodies (fir_tile_kernels.h).  x: the call's first sample (u8: byte); vec_in: x
// is 16-byte (u8: 4-byte) aligned.  LB is the plain loader's: ddc_load_thread keeps its own count in flight
template <bool U8>
struct DdcTile {
    using sample_t = float2;
    const void *x; long n_in; unsigned first_mod; const float2 *tab; unsigned L; int vec_in;
    template <bool STREAM, int LB, typename Put>
    RD_HD void load(int tid, long in0, int tile_in, Put &&put) const
    {
        const unsigned base = ddc_base(first_mod, (unsigned long long)in0, L); // wave-uniform: the workgroup's one modulo
        ddc_load_thread<U8, STREAM>(tid, 256, reinterpret_cast<const char *>(x) + in0 * (U8 ? 2 : 8), n_in - in0, tab + base, tile_in, vec_in != 0,
                                    (base & 1u) == 0, put);
    }
};

// the direct form: output i of a call, any K and D, no tile; idx0 = (first + i*D) mod L, one modulo, then wrap by compare
template <bool U8, bool FUSED>
RD_HD float2 ddc_direct_output(const void *x, unsigned idx0, const float2 *tab, unsigned L, const float *taps, int K)
{
    const float2 *xc = reinterpret_cast<const float2 *>(x);
    const unsigned char *xb = reinterpret_cast<const unsigned char *>(x);
    float2 acc = make_float2(0.f, 0.f);
    unsigned idx = idx0;
    for (int j = 0; j < K; ++j) {
        float2 m;
        if constexpr (U8) m = ddc_mix_u8(xb[2 * j], xb[2 * j + 1], tab[idx]);
        else m = cmul_rn(xc[j], tab[idx]);
        acc = mac<FUSED>(m, taps[j], acc);
        if (++idx == L) idx = 0;
    }
    return acc;
}

} // namespace redio
