// fir_tile.h -- the 256-lane tile shared by the FIR (fir_kernels.hip), the tuner (ddc_core.h) and the rational resampler
// (upfirdn_core.h): which decimations have a chunked form and with what shape, where a sample sits in the LDS image, how large the
// image is, the plain tile loader and the two store epilogues.  Everything about the tile is written down here once; the three
// plans name these functions.
//
// The tile.  A workgroup of 256 lanes produces 256 R outputs (the resampler: periods) from tile_in = (256 R - 1) D + W consecutive
// samples, W the window behind the last output's first sample.  A lane's stretch begins R D samples (the lane stride) after its
// neighbour's; where that stride is even the image holds one unused element per stride, so that 32 lanes start in 32 different bank
// pairs: sample n sits at tile_image_index(n, R D), lane `tid` begins at tile_lane_base(tid, R D).
//
// Host-compilable (tests/emu_fir, tests/emu_ddc and tests/emu_upfirdn run every thread of a workgroup on the CPU against an image of
// exactly the allocated size).
#pragma once
#include "redio_device.h"
#include <type_traits>

namespace redio {

constexpr long TILE_LDS_MAX = 150 * 1024; // bytes of LDS a tile may take; beyond it the plans' direct kernels run

// ---- the chunked forms: any tap count, decimation from this table ----------------------------------------------------------------
// outputs per lane R (0: no chunked form).  10: 1 or 4 outputs per lane ran 255 taps in 0.267 / 0.304 ms against 0.197
RD_HD constexpr int tile_r(long D) { return D == 1 ? 8 : (D >= 2 && D <= 5) ? 4 : (D == 8 || D == 10) ? 2 : 0; }
// whole-chunk size of fir_chunks (fir_chunks.h): a multiple of the lane stride wherever the image is padded (immediate window offsets)
RD_HD constexpr int tile_chw(long D) { return D == 3 ? 24 : (D == 5 || D == 10) ? 40 : 16; }
// what the kernels rely on at every row: R a power of two (the transpose index), whole chunks that begin on a lane stride, and a padded
// lane stride that is a multiple of four samples, so that the samples of one 16-byte load share one pad count and sit side by side
RD_HD constexpr bool tile_table_ok(int D)
{
    const int R = tile_r(D), lstr = R * D;
    return R > 0 && (R & (R - 1)) == 0 && (lstr % 2 != 0 || (tile_chw(D) % lstr == 0 && lstr % 4 == 0));
}
template <int D, typename F>
inline auto tile_call_d(F &&f)
{
    static_assert(tile_table_ok(D), "a row of the chunked table breaks what the kernels rely on");
    return f(std::integral_constant<int, D>{});
}
// a run-time decimation as a compile-time one: f(std::integral_constant<int, D>) for a D of the table, off_table for every other
template <typename Ret, typename F>
inline Ret tile_dispatch_d(long D, Ret off_table, F &&f)
{
    switch (D) {
    case 1: return tile_call_d<1>(f);
    case 2: return tile_call_d<2>(f);
    case 3: return tile_call_d<3>(f);
    case 4: return tile_call_d<4>(f);
    case 5: return tile_call_d<5>(f);
    case 8: return tile_call_d<8>(f);
    case 10: return tile_call_d<10>(f);
    default: return off_table;
    }
}

// ---- the image ---------------------------------------------------------------------------------------------------------------------
// image element of tile sample n at lane stride lstr
template <typename I>
RD_HD constexpr I tile_image_index(I n, I lstr) { return lstr % 2 == 0 ? n + n / lstr : n; }
// a lane's first element: tile_image_index(tid * lstr, lstr)
RD_HD constexpr int tile_lane_base(int tid, int lstr) { return tid * (lstr + (lstr % 2 == 0 ? 1 : 0)); }
// the output transpose: a lane writes its R results at a stride of R + 1 elements (conflict-free), so output e of the tile sits here
RD_HD constexpr int tile_transpose_index(int e, int R) { return (e / R) * (R + 1) + (e & (R - 1)); }
// samples a tile stages.  W: the window -- tile_window(K) for the chunked FIR and tuner (the taps run in whole chunks of 16), the
// resampler's Wp
RD_HD constexpr long tile_window(long K) { return (K + 15) / 16 * 16; }
RD_HD constexpr long tile_in(int R, long D, long W) { return (256L * R - 1) * D + W; }
// elements of the chunked FIR's and the tuner's LDS: four past the tile (the tail of a last 16-byte load; the loaders below write
// nothing there, the routes' pinned limits keep the term), the pad, two more, and never less than the output transpose that reuses it
RD_HD constexpr long tile_lds_elems(int R, long D, long W)
{
    const long e = tile_image_index(tile_in(R, D, W) + 4, (long)R * D) + 2;
    return e < 256L * (R + 1) ? 256L * (R + 1) : e;
}

// ---- 16-byte accesses behind a streaming policy (non-temporal where the samples go by once), plain ones in the host build ---------
#if defined(__HIPCC__)
typedef float fir_v4f __attribute__((ext_vector_type(4)));
#endif
template <bool STREAM>
RD_HD float4 tile_ld16(const float4 *p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (STREAM) {
        const fir_v4f v = __builtin_nontemporal_load(reinterpret_cast<const fir_v4f *>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    }
#endif
    return *p;
}
template <bool STREAM>
RD_HD void tile_st16(float4 *p, const float4 &q)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (STREAM) {
        __builtin_nontemporal_store(fir_v4f{q.x, q.y, q.z, q.w}, reinterpret_cast<fir_v4f *>(p));
        return;
    }
#endif
    *p = q;
}
// sample e of the 16 / sizeof(T) a 16-byte load holds
template <typename T>
RD_HD T tile_elem(const float4 &q, int e)
{
    const float f[4] = {q.x, q.y, q.z, q.w};
    if constexpr (sizeof(T) == 8) return T{f[2 * e], f[2 * e + 1]};
    else return f[e];
}

// ---- the plain loader ------------------------------------------------------------------------------------------------------------
// ONE thread `tid` of NT: tile sample n < tile_in from x[n] (the tile's first sample; zero beyond `left`, the samples the stream has
// from x on).  The sink: put(n, v) takes one sample; put(n, q) with a float4 takes the VEC = 16 / sizeof(T) samples of one load, n a
// multiple of VEC and all of them inside the tile.  Nothing at or beyond tile_in is ever put.
// vec_x: x is 16-byte aligned -- VEC samples per load, non-temporal with STREAM.  LB > 0: where the whole tile exists (workgroup-
// uniform) every lane keeps LB loads in flight with no bound check, the index clamped to the last load; LB == 0: the guarded loop alone.
// LB and STREAM are each kernel's own, as measured there.
template <typename T, bool STREAM, int LB, typename Put>
RD_HD void tile_load_thread(int tid, int NT, const T *x, long left, int tile_in, bool vec_x, Put &&put)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    auto put16 = [&](int v, const float4 &q) {
        const int n = v * VEC;
        if (n + VEC <= tile_in) {
            put(n, q);
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (n + e < tile_in) put(n + e, tile_elem<T>(q, e));
        }
    };
    if (vec_x) {
        const float4 *x4 = reinterpret_cast<const float4 *>(x);
        const int nv = (tile_in + VEC - 1) / VEC;
        int vfirst = tid;
        if constexpr (LB > 0) {
            if ((long)nv * VEC <= left) {
                for (; vfirst < nv; vfirst += LB * NT) {
                    float4 q[LB];
#pragma unroll
                    for (int b = 0; b < LB; ++b) {
                        const int v = vfirst + b * NT;
                        q[b] = tile_ld16<STREAM>(x4 + (v < nv ? v : nv - 1));
                    }
#pragma unroll
                    for (int b = 0; b < LB; ++b)
                        if (vfirst + b * NT < nv) put16(vfirst + b * NT, q[b]);
                }
            }
        }
#pragma unroll 4
        for (int v = vfirst; v < nv; v += NT) {
            const int n = v * VEC;
            if (n + VEC <= left) {
                put16(v, tile_ld16<STREAM>(x4 + v));
            } else {
#pragma unroll
                for (int e = 0; e < VEC; ++e)
                    if (n + e < tile_in) put(n + e, n + e < left ? x[n + e] : T{});
            }
        }
    } else {
#pragma unroll 4
        for (int n = tid; n < tile_in; n += NT) put(n, n < left ? x[n] : T{});
    }
}

// ---- the store epilogues ---------------------------------------------------------------------------------------------------------
// Lane-owned outputs: a lane's R consecutive results straight to y[o0 ...], the first n_out of which exist.  vec_y: y is 16-byte
// aligned (o0 * sizeof(T) is where R * sizeof(T) is a multiple of 16).
template <typename T, int R>
RD_HD void tile_store_lane(const T (&acc)[R], T *y, long o0, long n_out, bool vec_y)
{
    if (o0 + R <= n_out) {
        constexpr int BYTES = R * (int)sizeof(T);
        if constexpr (BYTES % 16 == 0) {
            if (vec_y) {
                float4 *y4 = reinterpret_cast<float4 *>(y + o0);
                const float *a = reinterpret_cast<const float *>(acc);
#pragma unroll
                for (int q = 0; q < BYTES / 16; ++q) y4[q] = make_float4(a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]);
                return;
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) y[o0 + r] = acc[r];
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (o0 + r < n_out) y[o0 + r] = acc[r];
    }
}

// Outputs through LDS, so that every store instruction writes 1 KiB of consecutive bytes.  ONE thread `tid` of NT: the tile's nel
// outputs (a multiple of 16 / sizeof(T)) to y, the tile's first output, `left` of which exist; output e of the tile is ys[index(e)]
// -- tile_transpose_index behind tile_transpose_put, the identity for the resampler's output tile.  vec_y: y is 16-byte aligned --
// 16-byte stores, non-temporal with STREAM.  Lds: a pointer to T, or what the emulators index in its place.
template <typename T, int R, typename Lds>
RD_HD void tile_transpose_put(Lds &&ys, int tid, const T (&acc)[R])
{
#pragma unroll
    for (int r = 0; r < R; ++r) ys[tid * (R + 1) + r] = acc[r]; // tile_transpose_index(tid * R + r, R)
}
template <typename T, bool STREAM, typename Lds, typename Index>
RD_HD void tile_store_thread(int tid, int NT, Lds &&ys, int nel, T *y, long left, bool vec_y, Index &&index)
{
    constexpr int VEC = 16 / (int)sizeof(T);
    for (int v = tid; v < nel / VEC; v += NT) {
        const int e0 = v * VEC;
        T o[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = ys[index(e0 + e)];
        if (vec_y && e0 + VEC <= left) {
            const float *f = reinterpret_cast<const float *>(o);
            tile_st16<STREAM>(reinterpret_cast<float4 *>(y) + v, make_float4(f[0], f[1], f[2], f[3]));
        } else {
#pragma unroll
            for (int e = 0; e < VEC; ++e)
                if (e0 + e < left) y[e0 + e] = o[e];
        }
    }
}

} // namespace redio
