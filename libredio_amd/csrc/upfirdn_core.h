// upfirdn_core.h -- the rational resampler (include/redio.h, redio_upfirdn_*): up by U, FIR, down by D as a polyphase FIR over the
// ORIGINAL samples.  Phase arithmetic, the route predicate, the phase program and the direct form; the tile's geometry, its loader and
// its store loop are the FIR's (fir_tile.h) with the window Wp in place of the padded tap count.
//
// Arithmetic contract (a stated design; the fold is dsputils::convolve's, src/dsputils/src/dsputils.rs:30-32):
//   z = x with U - 1 zeros behind every sample; y[i] = acc after acc = +0; for j = 0 .. K-1 ascending, ONLY where (i D + j) mod U == 0:
//   acc = mac(x[(i D + j) / U], h[j], acc)      mac: fir_core.h's (rounded multiply then rounded add, or fmaf with FUSED)
// Positions that hold a stuffed zero are skipped, never multiplied.  Phase by phase, with g = gcd(U, D), U' = U / g, D' = D / g and
// r in [0, U'):  j0(r) = (-(r D)) mod U,  s(r) = (r D + j0) / U,  K(r) = K > j0 ? ceil((K - j0) / U) : 0,  g_r[t] = h[j0 + U t] and
//   y[r + U' q] = the fold of x[s(r) + q D' + t] * g_r[t], t ascending
// -- a FIR decimating by D' with the sub-filter g_r, begun s(r) samples in; K(r) == 0 gives +0.  One period is U' outputs from D' new
// samples and reads the window Wp = ((U' - 1) D + K - 1) / U + 1 = max(1, max_r(s(r) + K(r))).
//
// Route 1 maps LANES TO PERIODS, not to consecutive outputs: in one phase every lane of a wave then uses the same sub-filter, so
// {s, K(r), taps} are wave-uniform, arrive by scalar loads, and the taps sit in SGPRs as in fir_chunks.h.  A 256-lane workgroup stages
// the tile_in(R, D', Wp) samples of its 256 R periods once (the padded image of fir_tile.h), walks the U' phases over it, and the
// outputs -- U' apart in memory within a phase -- leave through an LDS tile as contiguous 16-byte stores.
//
// Host-compilable (tests/emu_upfirdn runs every thread of a workgroup on the CPU).
#pragma once
#include "fir_tile.h"

namespace redio {

constexpr long UPFIRDN_MAX_UP = 65536;
constexpr long UPFIRDN_MAX_TAPS = 1L << 24;
constexpr long UPFIRDN_LDS_MAX = TILE_LDS_MAX;  // bytes: the chunked kernels' budget (fir_tile.h)
constexpr long UPFIRDN_LDS_WANT = 52 * 1024;  // three workgroups per CU (160 KiB): R shrinks to get there before it grows the tile
constexpr long UPFIRDN_TILED_MAX_PERIOD_OUT = 16; // route 1: the output tile is 256 R U' elements and the phase loop U' passes over the image

// one phase of the plan's device table: the window's start, the sub-filter's length and where its taps begin (in floats; every
// sub-filter zero-padded to a multiple of 16 floats, 64-byte aligned).  16 bytes: one aligned scalar load
struct UpfirdnPhase { int s, k, off, pad; };

RD_HD constexpr long upfirdn_gcd(long a, long b) { while (b) { const long t = a % b; a = b; b = t; } return a; }
RD_HD constexpr long upfirdn_period_out(long U, long D) { return U / upfirdn_gcd(U, D); } // U'
RD_HD constexpr long upfirdn_period_in(long U, long D) { return D / upfirdn_gcd(U, D); }  // D'
RD_HD constexpr long upfirdn_j0(long r, long U, long D) { return (U - (r * D) % U) % U; }
RD_HD constexpr long upfirdn_s(long r, long U, long D) { return (r * D + upfirdn_j0(r, U, D)) / U; }
RD_HD constexpr long upfirdn_k(long r, long K, long U, long D) { return K > upfirdn_j0(r, U, D) ? (K - upfirdn_j0(r, U, D) + U - 1) / U : 0; }
RD_HD constexpr long upfirdn_window(long K, long U, long D) { return ((upfirdn_period_out(U, D) - 1) * D + K - 1) / U + 1; } // Wp
// outputs of a stateless call on n samples: those whose K positions lie inside the n U positions of z
RD_HD constexpr unsigned long long upfirdn_nout(unsigned long long n, unsigned long long K, unsigned long long U, unsigned long long D)
{
    return n * U < K ? 0 : (n * U - K) / D + 1;
}

// the plan's two device arrays, built on the host: the phase table and the taps in polyphase order (Vec: a std::vector)
template <typename PhaseVec, typename TapVec>
inline void upfirdn_build(const float *taps, long K, long U, long D, PhaseVec &ph, TapVec &tp)
{
    ph.clear(); tp.clear();
    for (long r = 0; r < upfirdn_period_out(U, D); ++r) {
        const long j0 = upfirdn_j0(r, U, D), k = upfirdn_k(r, K, U, D);
        ph.push_back(UpfirdnPhase{(int)upfirdn_s(r, U, D), (int)k, (int)tp.size(), 0});
        for (long t = 0; t < k; ++t) tp.push_back(taps[j0 + U * t]);
        tp.resize((tp.size() + 15) / 16 * 16, 0.0f);
    }
    if (tp.empty()) tp.resize(16, 0.0f);
}

// ---- route 1's tile: 256 lanes x R periods of D' samples, the decimations of the chunked table; tile_in(R, D', Wp) samples --------------
// elements of the image (a multiple of four: the output tile behind it is 16-byte aligned for both sample types)
RD_HD constexpr long upfirdn_tile_in(int R, long Dp, long Wp) { return tile_in(R, Dp, Wp); }
RD_HD constexpr long upfirdn_img_elems(int R, long Dp, long Wp) { return (tile_image_index(upfirdn_tile_in(R, Dp, Wp), R * Dp) + 4) / 4 * 4; }
RD_HD constexpr long upfirdn_lds_elems(int R, long Up, long Dp, long Wp) { return upfirdn_img_elems(R, Dp, Wp) + 256L * R * Up; }
// periods per lane, decided on cf32 elements for both sample types: the largest of {4, 2, 1} inside UPFIRDN_LDS_WANT, else the largest
// inside UPFIRDN_LDS_MAX, else 0 (no tile).  Never more than the chunked FIR's R: at D' of 8 and 10 and R = 4 the window of 16 + 3 D' samples
// spilled scalar registers in the exact-fold cf32 kernels.  Off the table no tile runs (upfirdn_route); the second term only keeps the R that
// upfirdn_r reports there what it always was
RD_HD constexpr int upfirdn_r_max(long Dp) { return tile_r(Dp) ? (tile_r(Dp) < 4 ? tile_r(Dp) : 4) : (Dp >= 8 ? 2 : 4); }
RD_HD constexpr int upfirdn_r(long K, long U, long D)
{
    const long Up = upfirdn_period_out(U, D), Dp = upfirdn_period_in(U, D), Wp = upfirdn_window(K, U, D);
    for (int pass = 0; pass < 2; ++pass)
        for (int R = upfirdn_r_max(Dp); R >= 1; R /= 2)
            if (upfirdn_lds_elems(R, Up, Dp, Wp) * 8 <= (pass ? UPFIRDN_LDS_MAX : UPFIRDN_LDS_WANT)) return R;
    return 0;
}
// redio_upfirdn_route: 1 the phase-walking tiled kernel, 2 the direct one
RD_HD constexpr int upfirdn_route(long K, long U, long D)
{
    return tile_r(upfirdn_period_in(U, D)) != 0 && upfirdn_period_out(U, D) <= UPFIRDN_TILED_MAX_PERIOD_OUT && K <= (1 << 20) &&
                   upfirdn_r(K, U, D) != 0
               ? 1 : 2;
}

// Route 1's loader and store loop, ONE thread `tid` of NT each: the shared plain loader (fir_tile.h) with four loads in flight and a sink
// of single samples -- a lane stride of 2 or 4 samples (R = 1) does not keep the samples of one load side by side -- and the shared store
// loop over the contiguous output tile
template <typename T, bool STREAM, typename Put>
RD_HD void upfirdn_load_thread(int tid, int NT, const T *x, long left, int tile_in, bool vec_x, Put &&put)
{
    tile_load_thread<T, STREAM, 4>(tid, NT, x, left, tile_in, vec_x, [&](int n, auto v) {
        if constexpr (std::is_same_v<decltype(v), float4>) {
#pragma unroll
            for (int e = 0; e < 16 / (int)sizeof(T); ++e) put(n + e, tile_elem<T>(v, e));
        } else {
            put(n, v);
        }
    });
}
template <typename T, bool STREAM>
RD_HD void upfirdn_store_thread(int tid, int NT, const T *ys, int nel, T *y, long left, bool vec_y)
{
    tile_store_thread<T, STREAM>(tid, NT, ys, nel, y, left, vec_y, [](int e) { return e; });
}

// CH taps of one phase for the R periods of a lane: fir_chunk's program (fir_chunks.h) with the window begun `o` samples into the
// lane's stretch of the image, o = s(r) + the taps done so far: wave-uniform but NOT a multiple of the lane stride, so the pad count
// of window sample i is (o + i) / LSTR, a scalar division by a constant per read (fir_chunk's general form; its ALIGNED form cannot
// apply).  g: the phase's taps from the chunk's first on; base: the lane's first image element, tid * (LSTR + pad).
template <typename T, int D, int R, bool FUSED, int CH>
RD_HD void upfirdn_chunk(const T *xs, int base, int o, const float *__restrict__ g, T (&acc)[R])
{
    constexpr int WIN = CH + (R - 1) * D, LSTR = R * D;
    T xv[WIN];
    float h[CH];
#pragma unroll
    for (int i = 0; i < WIN; ++i) xv[i] = xs[base + tile_image_index(o + i, LSTR)]; // o + i is wave-uniform
#pragma unroll
    for (int j = 0; j < CH; ++j) h[j] = g[j];
#pragma unroll
    for (int i = 0; i < WIN; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = i - r * D;
            if (j >= 0 && j < CH) acc[r] = mac<FUSED>(xv[i], h[j], acc[r]);
        }
}

// all k taps of one phase: whole chunks of CHW, then the remainder's binary digits (as fir_chunks: no guarded tap, and no padded zero
// tap is ever multiplied -- 0 * inf and the sign of a zero sum are the contract's)
template <typename T, int D, int R, bool FUSED, int CHW = 16>
RD_HD void upfirdn_phase(const T *xs, int base, int s, int k, const float *__restrict__ g, T (&acc)[R])
{
    static_assert(CHW == 16 || CHW == 32, "the remainder's digits below");
    const int nfull = k / CHW;
    for (int c = 0; c < nfull; ++c) upfirdn_chunk<T, D, R, FUSED, CHW>(xs, base, s + c * CHW, g + c * CHW, acc);
    int j0 = nfull * CHW;
    const int rest = k - j0;
    if (CHW > 16 && (rest & 16)) { upfirdn_chunk<T, D, R, FUSED, 16>(xs, base, s + j0, g + j0, acc); j0 += 16; }
    if (rest & 8) { upfirdn_chunk<T, D, R, FUSED, 8>(xs, base, s + j0, g + j0, acc); j0 += 8; }
    if (rest & 4) { upfirdn_chunk<T, D, R, FUSED, 4>(xs, base, s + j0, g + j0, acc); j0 += 4; }
    if (rest & 2) { upfirdn_chunk<T, D, R, FUSED, 2>(xs, base, s + j0, g + j0, acc); j0 += 2; }
    if (rest & 1) upfirdn_chunk<T, D, R, FUSED, 1>(xs, base, s + j0, g + j0, acc);
}

// ONE thread of route 1 behind the loader: the U' phases of its R periods into the output tile ys (output e of the tile at ys[e],
// e = period * U' + phase).  The reads of ys by the store loop (tile_store_thread with the identity index) are consecutive; the writes here are R U' elements apart from lane to
// lane and take the bank conflicts that come with it (one write per output against K(r) / R window reads).
template <typename T, int D, int R, bool FUSED, int CHW>
RD_HD void upfirdn_phases_thread(const T *xs, T *ys, int tid, const UpfirdnPhase *__restrict__ ph, const float *__restrict__ taps, int Up)
{
    const int base = tile_lane_base(tid, R * D);
    for (int r = 0; r < Up; ++r) {
        const UpfirdnPhase p = ph[r]; // wave-uniform: a scalar load
        T acc[R];
#pragma unroll
        for (int q = 0; q < R; ++q) acc[q] = T{};
        upfirdn_phase<T, D, R, FUSED, CHW>(xs, base, p.s, p.k, taps + p.off, acc);
#pragma unroll
        for (int q = 0; q < R; ++q) ys[(tid * R + q) * Up + r] = acc[q];
    }
}

// route 2, output i of a call: one 64-bit division for the period and the phase, then the phase's fold straight from memory
template <typename T, bool FUSED>
RD_HD T upfirdn_direct_output(const T *x, long i, long Up, long Dp, const UpfirdnPhase *__restrict__ ph, const float *__restrict__ taps)
{
    const long q = i / Up;
    const UpfirdnPhase p = ph[i - q * Up];
    const T *w = x + q * Dp + p.s;
    const float *g = taps + p.off;
    T acc{};
    for (int t = 0; t < p.k; ++t) acc = mac<FUSED>(w[t], g[t], acc);
    return acc;
}

} // namespace redio
