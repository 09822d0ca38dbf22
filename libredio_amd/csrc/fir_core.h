// fir_core.h -- register-blocked valid-mode FIR (cross-correlation) for one lane.
//
// Arithmetic contract: dsputils::convolve, src/dsputils/src/dsputils.rs:30-32:
//   out[i] = fold(0.0, +) over j of u[i+j]*v[j]  -- taps NOT reversed, strict left-to-right order.
// Each accumulator below receives its products in ascending tap order j, so with FUSED=false
// (separate rounded multiply and add) a result is bit-identical to the reference fold, and with
// FUSED=true it is bit-identical to the same fold written with fmaf.  Decimation keeps out[D*i].
//
// Work split: a lane owns R consecutive kept outputs and walks its (R-1)*D+K input samples once;
// sample m feeds accumulator r with tap j = m - r*D.  The walk is fully unrolled so every tap index
// is a compile-time constant (taps are wave-uniform and live in SGPRs), and one LDS read feeds up to
// min(R, ceil(K/D)) multiply-adds.
//
// Host-compilable (tests/emu).
#pragma once
#include "fir_tile.h"
#include "redio_device.h"
#ifndef REDIO_EXP_ABLATE
#define REDIO_EXP_ABLATE 0
#endif
#include <type_traits>

namespace redio {

template <int K, int D, int R>
struct FirGeom {
    static constexpr int LSTR = R * D;             // input samples between neighbouring lanes
    static constexpr int SPAN = (R - 1) * D + K;   // input samples one lane touches
    static constexpr bool PAD = (LSTR % 2) == 0;   // LDS lane stride must be odd (in elements) so
                                                   // that 32 lanes hit 32 different bank pairs
    // LDS element index of tile-relative input sample n
    RD_HD static constexpr int lds_index(int n) { return tile_image_index(n, LSTR); }
    RD_HD static constexpr int tile_in(int tile_out) { return (tile_out - 1) * D + K; }
    RD_HD static constexpr int lds_elems(int tile_out) { return lds_index(tile_in(tile_out) - 1) + 1; }
};

// lane_first = tile-relative index of the first input sample of this lane's first output
// (= lane_slot * R * D).  xs is the LDS image written with FirGeom::lds_index.
template <typename T, int K, int D, int R, bool FUSED, typename LdsPtr, typename TapPtr>
RD_HD void fir_lane(LdsPtr xs, int lane_slot, TapPtr h, T (&acc)[R])
{
    using G = FirGeom<K, D, R>;
    const int base = lane_slot * (G::LSTR + (G::PAD ? 1 : 0)); // lds_index(lane_slot*LSTR)
#pragma unroll
    for (int m = 0; m < G::SPAN; ++m) {
        const T xv = xs[base + G::lds_index(m)];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = m - r * D;
            if (j >= 0 && j < K) acc[r] = mac<FUSED>(xv, h[j], acc[r]);
        }
    }
}

} // namespace redio

// ---------------------------------------------------------------------------------------------
// Variant for interleaved cf32 with 16-byte LDS reads: a lane's window is read two samples at a time
// (ds_read_b128), which needs every lane base 16-byte aligned and, for the four 16-lane groups of
// ds_read_b128 to be conflict-free, a lane stride S (in float2) with S/2 odd.
// ---------------------------------------------------------------------------------------------
namespace redio {

template <int K, int D, int R>
struct FirGeomV {
    static constexpr int LSTR = R * D;
    static_assert(LSTR % 2 == 0, "16-byte windows need an even lane stride");
    static constexpr int SPAN = (R - 1) * D + K;
    static constexpr int PADN = ((LSTR / 2) % 2 == 1) ? 0 : 2; // make (LSTR+PADN)/2 odd
    static constexpr int LANE_STRIDE = LSTR + PADN;
    RD_HD static constexpr int lds_index(int n) { return n + PADN * (n / LSTR); }
    RD_HD static constexpr int tile_in(int tile_out) { return (tile_out - 1) * D + K; }
    // float2 elements, rounded up to an even count (whole float4s)
    RD_HD static constexpr int lds_elems(int tile_out) { return (lds_index(tile_in(tile_out) - 1) + 2) & ~1; }
};

// xs4: the LDS image viewed as 16-byte elements (two cf32 samples each), written with
// FirGeomV::lds_index.  The window is consumed in chunks of CH reads with the next chunk's reads
// issued before the current chunk's multiply-adds and a scheduling barrier between chunks: LDS
// latency hides behind ~100 packed FMAs while only two chunks of samples are ever live in
// registers (an unconstrained schedule hoists dozens of reads and spills).
template <int N, typename F>
RD_HD void fir_static_for(F &&f)
{
    if constexpr (N > 0) {
        fir_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// Taps needed by chunk c: samples m in [2*CH*c, 2*CH*(c+1)) feed output r with tap j = m - r*D, so
// j spans [2*CH*c - (R-1)*D, 2*CH*(c+1) - 1], clipped to [0, K).
template <int K, int D, int R, int CH>
struct FirChunkTaps {
    static constexpr int NT = 2 * CH + (R - 1) * D; // taps a chunk can touch
    RD_HD static constexpr int lo(int c) { return 2 * CH * c - (R - 1) * D; }
};

// A caller's own work issued between the chunks of a window (the chain kernel: the previous block's transform, piece by piece):
// hook(integral_constant<int, c>) runs once per chunk c = 0 ... fir_num_chunks - 1, after the next chunk's reads are requested and
// before this chunk's multiply-adds, inside the chunk's scheduling region.  FirNoHook: nothing.
struct FirNoHook {
    template <typename C>
    RD_HD void operator()(C) const {}
};
template <int K, int D, int R, int CH>
RD_HD constexpr int fir_num_chunks() { return ((FirGeomV<K, D, R>::SPAN + 1) / 2 + CH - 1) / CH; }

template <int c, int K, int D, int R, bool FUSED, int CH, typename Q, typename Lds4Ptr, typename TapPtr, typename Hook>
RD_HD void fir_chunks_v(Lds4Ptr xs4, int base4, TapPtr h, Q (&q)[2][CH],
                        float (&hb)[2][FirChunkTaps<K, D, R, CH>::NT], float2 (&acc)[R], Hook &hook)
{
    using G = FirGeomV<K, D, R>;
    using T = FirChunkTaps<K, D, R, CH>;
    constexpr int NRD = (G::SPAN + 1) / 2; // 16-byte reads in a window
    constexpr int NCH = (NRD + CH - 1) / CH;
    if constexpr (c < NCH) {
        // everything this chunk consumes was requested one chunk ago; naming one tap and one sample
        // here makes the single lgkmcnt(0) land BEFORE the next chunk's requests are issued
        RD_PIN_SV(hb[c & 1][T::NT - 1], q[c & 1][0]);
        fir_static_for<CH>([&](auto I) { // the next chunk's samples (LDS) ...
            constexpr int i = (c + 1) * CH + I.value;
#if REDIO_EXP_ABLATE == 1 // timing-only experiment (tools/ablate.sh), never in the product build: half the window reads
            if constexpr (i < NRD && (I.value & 1)) q[(c + 1) & 1][I.value] = q[(c + 1) & 1][I.value - 1];
            else
#endif
            if constexpr (i < NRD) q[(c + 1) & 1][I.value] = xs4[base4 + G::lds_index(2 * i) / 2];
        });
        fir_static_for<T::NT>([&](auto J) { // ... and taps (scalar cache)
            constexpr int j = T::lo(c + 1) + J.value;
            if constexpr (c + 1 < NCH && j >= 0 && j < K) hb[(c + 1) & 1][J.value] = h[j];
        });
        hook(std::integral_constant<int, c>{});
        fir_static_for<CH>([&](auto I) {
            constexpr int m = 2 * (c * CH + I.value);
            if constexpr (m < G::SPAN) {
                const Q v = q[c & 1][I.value];
                const float2 x0 = make_float2(v.x, v.y), x1 = make_float2(v.z, v.w);
                fir_static_for<R>([&](auto RR) {
                    constexpr int r = RR.value;
#if REDIO_EXP_ABLATE == 2 // timing-only experiment: half the multiply-adds (two of the four accumulators)
                    if constexpr (r & 1) return;
#endif
                    constexpr int j0 = m - r * D, j1 = m + 1 - r * D;
                    if constexpr (j0 >= 0 && j0 < K) acc[r] = mac<FUSED>(x0, hb[c & 1][j0 - T::lo(c)], acc[r]);
                    if constexpr (j1 >= 0 && j1 < K && m + 1 < G::SPAN) acc[r] = mac<FUSED>(x1, hb[c & 1][j1 - T::lo(c)], acc[r]);
                });
            }
        });
        // pin the accumulators: without a data dependency the compiler sinks every multiply-add below
        // the last read and the chunking is lost
#pragma unroll
        for (int r = 0; r < R; ++r) RD_PIN_F2(acc[r]);
        RD_SCHED_BARRIER();
        fir_chunks_v<c + 1, K, D, R, FUSED, CH>(xs4, base4, h, q, hb, acc, hook);
    }
}

template <int K, int D, int R, bool FUSED, int CH = 8 /* 16-byte reads per chunk */, typename Lds4Ptr, typename TapPtr, typename Hook>
RD_HD void fir_lane_v(Lds4Ptr xs4, int lane_slot, TapPtr h, float2 (&acc)[R], Hook &&hook)
{
    using G = FirGeomV<K, D, R>;
    using Q = typename std::remove_cv<typename std::remove_reference<decltype(xs4[0])>::type>::type;
    constexpr int NRD = (G::SPAN + 1) / 2;
    using T = FirChunkTaps<K, D, R, CH>;
    const int base4 = lane_slot * (G::LANE_STRIDE / 2);
    Q q[2][CH];
    float hb[2][T::NT];
    fir_static_for<T::NT>([&](auto J) { // last slot is always written so that it can be pinned
        constexpr int j = T::lo(0) + J.value;
        hb[0][J.value] = (j >= 0 && j < K) ? h[j] : 0.0f;
        hb[1][J.value] = 0.0f;
    });
    fir_static_for<CH>([&](auto I) {
        constexpr int i = I.value;
        if constexpr (i < NRD) q[0][i] = xs4[base4 + G::lds_index(2 * i) / 2];
    });
    fir_chunks_v<0, K, D, R, FUSED, CH>(xs4, base4, h, q, hb, acc, hook);
}
template <int K, int D, int R, bool FUSED, int CH = 8, typename Lds4Ptr, typename TapPtr>
RD_HD void fir_lane_v(Lds4Ptr xs4, int lane_slot, TapPtr h, float2 (&acc)[R])
{
    fir_lane_v<K, D, R, FUSED, CH>(xs4, lane_slot, h, acc, FirNoHook{});
}

// ---------------------------------------------------------------------------------------------
// The same lane program for PALINDROMIC taps (h[j] and h[K-1-j] the same 32-bit pattern, which every
// lpf_corrected design is): the ceil(K/2) distinct values stay in scalar registers for the life of the
// wave as aligned 64-bit pairs, loaded once before the sub-tile loop.  Tap j is element
// e = min(j, K-1-j): pair e/2, low word for even e, high word for odd e, selected by op_sel on the packed
// multiply-add itself -- no per-chunk staging copy, no scalar move, and no scalar load inside the loop,
// so the window's ds_read_b128 are the only counted (in-order) requests and are waited on one by one.
// Samples are taken in ascending order and the live outputs of a sample in turn (r ascending), so each
// output still receives its products in ascending tap order with the same rounding steps: same bits.
// ---------------------------------------------------------------------------------------------
template <int K>
struct FirTapsResident {
    static constexpr int NE = (K + 1) / 2;  // distinct tap values
    static constexpr int NP = (NE + 1) / 2; // aligned pairs (the odd one out pairs with its mirror: index NE <= K-1 for K >= 3)
    static_assert(K >= 3, "a pair never reads past the taps");
    RD_HD static constexpr int elem(int j) { return j < K - 1 - j ? j : K - 1 - j; }
    unsigned long long p[NP]; // (h[2i], h[2i+1]) as stored: low word first
};

struct FirNoResidentTaps {}; // what an any-taps kernel carries in that place: nothing

// h: 8-byte aligned, wave-uniform.  Device: each pair is made opaque in a scalar register pair, so it is neither
// re-fetched nor rebuilt inside the loop.  All pairs are requested before the first is made opaque: naming a pair waits for it,
// and a wait per pair is NP scalar-cache latencies in a row at the head of every wave instead of one.
template <int K, typename TapPtr>
RD_HD void fir_taps_resident_load(FirTapsResident<K> &t, TapPtr h)
{
#if defined(__HIP_DEVICE_COMPILE__) && !(defined(REDIO_EXP_SEAM) && !(REDIO_EXP_SEAM & 8))
    fir_static_for<FirTapsResident<K>::NP>([&](auto I) {
        typedef unsigned long long u64a __attribute__((may_alias));
        t.p[I.value] = reinterpret_cast<const u64a *>(&h[0])[I.value];
    });
#pragma unroll
    for (int i = 0; i < FirTapsResident<K>::NP; ++i) asm volatile("" : "+s"(t.p[i]));
#else
    fir_static_for<FirTapsResident<K>::NP>([&](auto I) {
        constexpr int i = I.value;
#if defined(__HIP_DEVICE_COMPILE__) // the measurement build's parent form (REDIO_EXP_SEAM without bit 3): a wait per pair
        typedef unsigned long long u64a __attribute__((may_alias));
        t.p[i] = reinterpret_cast<const u64a *>(&h[0])[i];
        asm volatile("" : "+s"(t.p[i]));
#else
        unsigned lo, hi;
        const float a = h[2 * i], b = h[2 * i + 1];
        __builtin_memcpy(&lo, &a, 4);
        __builtin_memcpy(&hi, &b, 4);
        t.p[i] = (unsigned long long)lo | ((unsigned long long)hi << 32);
#endif
    });
#endif
}

// live outputs of window sample m: r in [r_lo(m), r_hi(m)], tap j = m - r*D in [0, K)
template <int K, int D, int R>
struct FirLive {
    RD_HD static constexpr int lo(int m) { return m - (K - 1) <= 0 ? 0 : (m - (K - 1) + D - 1) / D; }
    RD_HD static constexpr int hi(int m) { return m / D < R - 1 ? m / D : R - 1; }
};

#if defined(__HIP_DEVICE_COMPILE__)
typedef redio_v2f fir_acc_t; // one output (re, im) as ONE aligned 64-bit register pair
#else
typedef float2 fir_acc_t;
#endif

// What one 16-byte window read (samples m0 and m0 + 1) feeds: slot k = 4 * i + r is sample m0 + i into output r.
template <int m0, int K, int D, int R, bool TWO /* sample m0 + 1 is inside the window */>
struct FirReadPlan {
    using L = FirLive<K, D, R>;
    using T = FirTapsResident<K>;
#if REDIO_EXP_ABLATE == 2 // timing-only experiment (tools/ablate.sh): half the multiply-adds (two of the four accumulators), as in fir_chunks_v
    RD_HD static constexpr bool live(int k) { return !(k & 1) && (k < 4 || TWO) && (k & 3) >= L::lo(m0 + k / 4) && (k & 3) <= L::hi(m0 + k / 4) && (k & 3) < R; }
#else
    RD_HD static constexpr bool live(int k) { return (k < 4 || TWO) && (k & 3) >= L::lo(m0 + k / 4) && (k & 3) <= L::hi(m0 + k / 4) && (k & 3) < R; }
#endif
    RD_HD static constexpr int elem(int k) { return live(k) ? T::elem(m0 + k / 4 - (k & 3) * D) : 0; }
    RD_HD static constexpr int pair(int k) { return elem(k) / 2; }
    RD_HD static constexpr unsigned en() { unsigned v = 0; for (int k = 0; k < 8; ++k) v |= (live(k) ? 1u : 0u) << k; return v; }
    RD_HD static constexpr unsigned hi() { unsigned v = 0; for (int k = 0; k < 8; ++k) v |= (unsigned)(elem(k) & 1) << k; return v; }
    // FUSED: slots whose accumulator was written by the packed operation just before them (the previous live slot, or the last
    // one of the previous read; the very first sample counts too: it follows the compiler's own initialisation)
    RD_HD static constexpr unsigned nop_fused()
    {
        unsigned v = 0;
        int prev = m0 == 0 ? 0 : L::hi(m0 - 1);
        for (int k = 0; k < 8; ++k)
            if (live(k)) { if ((k & 3) == prev) v |= 1u << k; prev = k & 3; }
        return v;
    }
    // exact: bit i = sample m0 + i has ONE live output, so its add would directly follow its multiply
    RD_HD static constexpr unsigned nop_exact()
    {
        unsigned v = 0;
        for (int i = 0; i < 2; ++i) {
            int n = 0;
            for (int r = 0; r < 4; ++r) n += live(4 * i + r) ? 1 : 0;
            if (n == 1) v |= 1u << i;
        }
        return v;
    }
};

#if defined(__HIP_DEVICE_COMPILE__)
// The packed operations of ONE 16-byte read as ONE inline-assembly statement: acc[r] <- acc[r] + x_i * tap for the live slots, samples
// in ascending order, the outputs of a sample in turn.  The slots a read does not have are assembled away (.if on the masks, which are
// compile-time constants); their operands name registers that are live anyway.  One statement per read, so the compiler's wait for
// that read (by count) is what separates two statements.
// Inline assembly hides the instructions from the compiler's hazard pass: on gfx950 a packed-f32 result needs one wait state before
// a vector instruction reads it, so no two DEPENDENT packed operations may be adjacent.  How that is guaranteed:
//   FUSED: consecutive multiply-adds of a sample write different accumulators; where a slot's accumulator is the one the packed
//          operation right before it wrote (one live output at the window's ends, the hand-over from sample to sample when the
//          live ranges touch in one output, and across two statements, where the compiler may put nothing in between) the statement
//          itself has an `s_nop 0` in front of that slot (FirReadPlan::nop_fused).
//   exact: per sample, all multiplies come first and then the adds, so with two or more live outputs a product's add is at least
//          two instructions behind its multiply and behind the previous add of its accumulator; with ONE live output an `s_nop 0`
//          sits between the multiply and the add (nop_exact).  A sample begins with multiplies, which read no accumulator.
//   fir_lane_v_res names the four accumulators in a statement of their own, followed by a wait state, before the first read's
//   statement (the compiler's initialisation of them is then complete), and ends with one more `s_nop 0` before compiler code reads them.
#define RD_FMA_SLOT(k, r, i)                                                                                             \
    ".if (%[nb] >> " #k ") & 1\ns_nop 0\n.endif\n"                                                                      \
    ".if (%[en] >> " #k ") & 1\n.if (%[hi] >> " #k ") & 1\n"                                                            \
    "v_pk_fma_f32 %[a" #r "], %[x" #i "], %[t" #k "], %[a" #r "] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n.else\n"               \
    "v_pk_fma_f32 %[a" #r "], %[x" #i "], %[t" #k "], %[a" #r "] op_sel:[0,0,0] op_sel_hi:[1,0,1]\n.endif\n.endif\n"
#define RD_MUL_SLOT(k, r, i)                                                                                             \
    ".if (%[en] >> " #k ") & 1\n.if (%[hi] >> " #k ") & 1\n"                                                            \
    "v_pk_mul_f32 %[d" #r "], %[x" #i "], %[t" #k "] op_sel:[0,1] op_sel_hi:[1,1]\n.else\n"                               \
    "v_pk_mul_f32 %[d" #r "], %[x" #i "], %[t" #k "] op_sel:[0,0] op_sel_hi:[1,0]\n.endif\n.endif\n"
#define RD_ADD_SLOT(k, r) ".if (%[en] >> " #k ") & 1\nv_pk_add_f32 %[a" #r "], %[a" #r "], %[d" #r "]\n.endif\n"
#define RD_ONE_NOP(i) ".if (%[nb] >> " #i ") & 1\ns_nop 0\n.endif\n"
template <int m0, int K, int D, int R, bool FUSED, bool TWO>
RD_D void fir_read_res(redio_v2f x0, redio_v2f x1, const FirTapsResident<K> &t, redio_v2f (&a)[R])
{
    static_assert(R == 4, "four accumulators per lane");
    using P = FirReadPlan<m0, K, D, R, TWO>;
    if constexpr (FUSED)
        asm volatile(RD_FMA_SLOT(0, 0, 0) RD_FMA_SLOT(1, 1, 0) RD_FMA_SLOT(2, 2, 0) RD_FMA_SLOT(3, 3, 0)
                     RD_FMA_SLOT(4, 0, 1) RD_FMA_SLOT(5, 1, 1) RD_FMA_SLOT(6, 2, 1) RD_FMA_SLOT(7, 3, 1)
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3])
                     : [x0] "v"(x0), [x1] "v"(x1), [t0] "s"(t.p[P::pair(0)]), [t1] "s"(t.p[P::pair(1)]), [t2] "s"(t.p[P::pair(2)]),
                       [t3] "s"(t.p[P::pair(3)]), [t4] "s"(t.p[P::pair(4)]), [t5] "s"(t.p[P::pair(5)]), [t6] "s"(t.p[P::pair(6)]),
                       [t7] "s"(t.p[P::pair(7)]), [en] "i"(P::en()), [hi] "i"(P::hi()), [nb] "i"(P::nop_fused()));
    else {
        redio_v2f d0, d1, d2, d3;
        asm volatile(RD_MUL_SLOT(0, 0, 0) RD_MUL_SLOT(1, 1, 0) RD_MUL_SLOT(2, 2, 0) RD_MUL_SLOT(3, 3, 0) RD_ONE_NOP(0)
                     RD_ADD_SLOT(0, 0) RD_ADD_SLOT(1, 1) RD_ADD_SLOT(2, 2) RD_ADD_SLOT(3, 3)
                     RD_MUL_SLOT(4, 0, 1) RD_MUL_SLOT(5, 1, 1) RD_MUL_SLOT(6, 2, 1) RD_MUL_SLOT(7, 3, 1) RD_ONE_NOP(1)
                     RD_ADD_SLOT(4, 0) RD_ADD_SLOT(5, 1) RD_ADD_SLOT(6, 2) RD_ADD_SLOT(7, 3)
                     : [a0] "+v"(a[0]), [a1] "+v"(a[1]), [a2] "+v"(a[2]), [a3] "+v"(a[3]), [d0] "=&v"(d0), [d1] "=&v"(d1), [d2] "=&v"(d2),
                       [d3] "=&v"(d3)
                     : [x0] "v"(x0), [x1] "v"(x1), [t0] "s"(t.p[P::pair(0)]), [t1] "s"(t.p[P::pair(1)]), [t2] "s"(t.p[P::pair(2)]),
                       [t3] "s"(t.p[P::pair(3)]), [t4] "s"(t.p[P::pair(4)]), [t5] "s"(t.p[P::pair(5)]), [t6] "s"(t.p[P::pair(6)]),
                       [t7] "s"(t.p[P::pair(7)]), [en] "i"(P::en()), [hi] "i"(P::hi()), [nb] "i"(P::nop_exact()));
    }
}
#undef RD_FMA_SLOT
#undef RD_MUL_SLOT
#undef RD_ADD_SLOT
#undef RD_ONE_NOP
#else
// the plain C++ form of the same order (host builds)
template <int m0, int K, int D, int R, bool FUSED, bool TWO>
RD_HD void fir_read_res(float2 x0, float2 x1, const FirTapsResident<K> &t, float2 (&a)[R])
{
    using P = FirReadPlan<m0, K, D, R, TWO>;
    for (int k = 0; k < 8; ++k) {
        if (!P::live(k)) continue;
        const int el = P::elem(k);
        const unsigned w = (unsigned)(t.p[el / 2] >> (32 * (el & 1)));
        float h;
        __builtin_memcpy(&h, &w, 4);
        a[k & 3] = mac<FUSED>(k < 4 ? x0 : x1, h, a[k & 3]);
    }
}
#endif

template <int c, int K, int D, int R, bool FUSED, int CH, typename Q, typename Lds4Ptr, typename Hook>
RD_HD void fir_chunks_res(Lds4Ptr xs4, int base4, const FirTapsResident<K> &t, Q (&q)[2][CH], fir_acc_t (&acc)[R], Hook &hook)
{
    using G = FirGeomV<K, D, R>;
    constexpr int NRD = (G::SPAN + 1) / 2; // 16-byte reads in a window
    constexpr int NCH = (NRD + CH - 1) / CH;
    if constexpr (c < NCH) {
        // the next chunk's samples are requested before this chunk's arithmetic; naming this chunk's first sample in an ordered
        // statement keeps the requests behind the wait for it (a wait by count: LDS reads return in order)
        RD_PIN_V(q[c & 1][0]);
        fir_static_for<CH>([&](auto I) {
            constexpr int i = (c + 1) * CH + I.value;
#if REDIO_EXP_ABLATE == 1 // timing-only experiment (tools/ablate.sh), never in the product build: half the window reads, as in fir_chunks_v
            if constexpr (i < NRD && (I.value & 1)) q[(c + 1) & 1][I.value] = q[(c + 1) & 1][I.value - 1];
            else
#endif
            if constexpr (i < NRD) q[(c + 1) & 1][I.value] = xs4[base4 + G::lds_index(2 * i) / 2];
        });
        hook(std::integral_constant<int, c>{});
        fir_static_for<CH>([&](auto I) {
            constexpr int m = 2 * (c * CH + I.value);
            if constexpr (m < G::SPAN) {
                const Q v = q[c & 1][I.value];
#if defined(__HIP_DEVICE_COMPILE__)
                const fir_acc_t x0 = __builtin_shufflevector(v, v, 0, 1), x1 = __builtin_shufflevector(v, v, 2, 3);
#else
                const fir_acc_t x0 = make_float2(v.x, v.y), x1 = make_float2(v.z, v.w);
#endif
                fir_read_res<m, K, D, R, FUSED, (m + 1 < G::SPAN)>(x0, x1, t, acc);
            }
        });
        RD_SCHED_BARRIER();
        fir_chunks_res<c + 1, K, D, R, FUSED, CH>(xs4, base4, t, q, acc, hook);
    }
}

// fir_lane_v with resident palindromic taps (PRECONDITION: the taps t was loaded from are bit-palindromic); xs4 on the device is a
// view of 16-byte vectors of four floats
template <int K, int D, int R, bool FUSED, int CH = 8, typename Lds4Ptr, typename Hook>
RD_HD void fir_lane_v_res(Lds4Ptr xs4, int lane_slot, const FirTapsResident<K> &t, float2 (&acc)[R], Hook &&hook)
{
    using G = FirGeomV<K, D, R>;
    using Q = typename std::remove_cv<typename std::remove_reference<decltype(xs4[0])>::type>::type;
    constexpr int NRD = (G::SPAN + 1) / 2;
    const int base4 = lane_slot * (G::LANE_STRIDE / 2);
    Q q[2][CH];
    fir_static_for<CH>([&](auto I) {
        constexpr int i = I.value;
        if constexpr (i < NRD) q[0][i] = xs4[base4 + G::lds_index(2 * i) / 2];
    });
    fir_acc_t a[R];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = fir_acc_t{acc[r].x, acc[r].y};
    static_assert(R == 4, "four accumulators per lane");
    asm volatile("s_nop 0" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3])); // initialised, and one wait state old, before the first read's statement
#else
    for (int r = 0; r < R; ++r) a[r] = acc[r];
#endif
    fir_chunks_res<0, K, D, R, FUSED, CH>(xs4, base4, t, q, a, hook);
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("s_nop 0"); // the last packed result, one wait state ahead of the compiler's first reader
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = make_float2(a[r].x, a[r].y);
#else
    for (int r = 0; r < R; ++r) acc[r] = a[r];
#endif
}
template <int K, int D, int R, bool FUSED, int CH = 8, typename Lds4Ptr>
RD_HD void fir_lane_v_res(Lds4Ptr xs4, int lane_slot, const FirTapsResident<K> &t, float2 (&acc)[R])
{
    fir_lane_v_res<K, D, R, FUSED, CH>(xs4, lane_slot, t, acc, FirNoHook{});
}

} // namespace redio

// ---------------------------------------------------------------------------------------------
// REAL samples without decimation, two outputs per packed multiply-add (round 6).  A lane owns R consecutive outputs as R/2
// accumulator PAIRS (out[2p], out[2p+1]); tap j feeds pair p with the sample pair (x[2p + j], x[2p + 1 + j]) -- one v_pk_fma_f32 (or
// v_pk_mul + v_pk_add) whose two halves are two outputs' strict left folds (dsputils.rs:31), each still receiving its products in
// ascending tap order.  A pair that starts on an odd sample is no aligned 64-bit register pair of the even ones: the scalar lane
// program above leaves that to the compiler, which builds them with one v_mov per pair (49 moves per 252 packed multiply-adds in
// the 63-tap kernel).  Here the tile is stored TWICE in LDS, as E2[m] = (x[2m], x[2m+1]) and as O2[m] = (x[2m+1], x[2m+2]), so that
// every pair is one aligned 8-byte read and the multiply-adds are the only vector instructions of the body.
// Image element m (a float2) of either copy sits at lds_index(m): lane stride R/2 float2, one pad element per lane when that is even
// (odd stride: the 32 lanes of a ds_read_b64 hit 32 different bank pairs).
// ---------------------------------------------------------------------------------------------
namespace redio {

template <int K, int R>
struct FirGeomPairs {
    static_assert(R % 2 == 0, "pairs of outputs");
    static constexpr int LSTR = R / 2;                    // float2 elements between neighbouring lanes
    static constexpr bool PAD = (LSTR % 2) == 0;
    static constexpr int LANE_STRIDE = LSTR + (PAD ? 1 : 0);
    static constexpr int NPAIR = R / 2 + (K - 1) / 2 + ((K - 1) % 2 ? 1 : 0); // pair slots m one lane reads from EACH copy: m < R/2 + ceil((K-1)/2)
    RD_HD static constexpr int lds_index(int m) { return tile_image_index(m, LSTR); }
    RD_HD static constexpr int tile_in(int tile_out) { return tile_out - 1 + K; }
    // float2 elements of ONE copy for a tile of tile_out outputs: the tile is staged in whole 16-byte loads (four samples = two
    // elements of either copy), so a copy holds 2 * ceil(tile_in / 4) elements
    RD_HD static constexpr int copy_elems(int tile_out) { return lds_index(2 * ((tile_in(tile_out) + 3) / 4) - 1) + 1; }
};

// e2 / o2: the two copies of the image (float2 views); acc[p] = (out[2p], out[2p+1]) of this lane
template <int K, int R, bool FUSED, typename LdsPtr, typename TapPtr>
RD_HD void fir_lane_pairs(LdsPtr e2, LdsPtr o2, int lane_slot, TapPtr h, float2 (&acc)[R / 2])
{
    using G = FirGeomPairs<K, R>;
    const int base = lane_slot * G::LANE_STRIDE;
#pragma unroll
    for (int m = 0; m < G::NPAIR; ++m) {
        const float2 e = e2[base + G::lds_index(m)]; // (x[2m], x[2m+1]) relative to the lane's first output
        const float2 o = o2[base + G::lds_index(m)]; // (x[2m+1], x[2m+2])
#pragma unroll
        for (int p = 0; p < R / 2; ++p) {
            const int j = 2 * (m - p);
            if (j >= 0 && j < K) acc[p] = mac<FUSED>(e, h[j], acc[p]);
            if (j + 1 >= 0 && j + 1 < K) acc[p] = mac<FUSED>(o, h[j + 1], acc[p]);
        }
    }
}

} // namespace redio
