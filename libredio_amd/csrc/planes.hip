// planes.hip -- layout change between the channelizer's output and the batched resampler's input:
//   rows    cf32 [nrows][nchan]            one row of channel samples per output time (redio_pfb_enqueue)
//   planes  f32  [2*nchan][plane_stride]   plane 2c = Re of channel c, plane 2c + 1 = Im; one contiguous mono stream per plane
//                                          (redio_src_enqueue's [nchan][in_stride] with twice the channels)
// Seen as 32-bit words the rows are a matrix [nrows][NP], NP = 2*nchan, without gaps, and the planes are its transpose with a leading
// stride.  Pure data movement: words travel as uint32 (NaN payloads and -0 arrive unchanged).
//
// One workgroup of 256 lanes moves a tile of TF consecutive frames x tp <= 64 consecutive planes through LDS:
//   * NP <= 64: tp = NP and the tile's row side is ONE contiguous run of TF*NP words (TF = the multiple of 64 that brings the tile to
//     about 4096 words); NP > 64: TF = 64 and the row side is 64 runs of tp words.  16-byte lanes when the row base is 16-byte aligned
//     (and NP % 4 == 0 where the tile does not span whole rows); else 4-byte lanes.
//   * the plane side is tp runs of TF consecutive frames (whole tiles: 256 bytes or more per plane).  16-byte lanes when the plane
//     base is 16-byte aligned and plane_stride % 4 == 0; 4-byte lanes otherwise and for the quads the last tile cuts.
//   * LDS image [plane][TF + 1] words (at most 64 * 65 = 4160 words = 16.25 KiB: nine workgroups fit a CU's 160 KiB; the eight that
//     its wave slots take are resident).  The odd pitch puts the 4-byte lanes of either side on 32 different banks.  A lane of a
//     16-byte access moves its four words with four ds_{read,write}_b32, lanes 4 words apart: two lanes per bank, which doubles the
//     LDS-array cycles of the instruction to what its register transfer takes anyway (4 cycles for ds_write_b32) -- about 500 LDS
//     cycles per tile against some 2500 cycles of the tile's 32 KiB at a CU's share of HBM.
// Messages beyond the caches write with non-temporal stores (nothing re-reads them soon); smaller ones keep the default policy,
// their consumer usually runs next.
#include "../../include/redio.h"
#include "redio_internal.h"

namespace redio {

enum { PLANES_TP = 64, PLANES_WORDS = 4096, PLANES_LDS = PLANES_TP * (PLANES_WORDS / PLANES_TP + 1) };
typedef uint32_t planes_v4u __attribute__((ext_vector_type(4)));

// frames per tile for tp_full = min(NP, 64) planes: tp_full * (TF + 1) <= PLANES_LDS
static inline int planes_tile_frames(int tp_full)
{
    const int tf = (PLANES_WORDS / tp_full) & ~63;
    return tf < 64 ? 64 : tf;
}

template <bool NT>
__device__ __forceinline__ void planes_st4(uint32_t *p, planes_v4u v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<planes_v4u *>(p));
    else *reinterpret_cast<planes_v4u *>(p) = v;
}
template <bool NT>
__device__ __forceinline__ void planes_st1(uint32_t *p, uint32_t v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// exact quotient by a multiply: m = ceil(2^32 / d), 2 <= d; q = i / d for i * d < 2^32 (tile indices are below 4160, d at most 2048)
__device__ __forceinline__ unsigned planes_magic(unsigned d) { return 0xFFFFFFFFu / d + 1u; }

struct PlanesTile {
    long f0;     // first frame
    int tf, tp;  // frames and planes in this tile
    int p0;      // first plane
    int pitch;   // LDS words per plane
    int TF;      // frames of a full tile
};

// row side: tile word i = (frame i / tp, plane i % tp) at rows[(f0 + f) * NP + p0 + p]; four consecutive words of a 16-byte lane are
// consecutive in memory (NP <= 64: the whole tile is; else tp % 4 == 0 and a quad stays inside a frame's run)
template <bool TO_LDS, bool NT>
__device__ __forceinline__ void planes_row_side(uint32_t *rows, int NP, const PlanesTile &t, uint32_t *lds, bool vec)
{
    const int tid = threadIdx.x, n = t.tf * t.tp;
    const unsigned m = planes_magic((unsigned)t.tp);
    const int nv = vec ? (n & ~3) : 0;
    for (int i = 4 * tid; i < nv; i += 4 * 256) {
        int f[4], p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            f[k] = (int)__umulhi((unsigned)(i + k), m);
            p[k] = i + k - f[k] * t.tp;
        }
        uint32_t *g = rows + (t.f0 + f[0]) * NP + t.p0 + p[0];
        if constexpr (TO_LDS) {
            const planes_v4u v = *reinterpret_cast<const planes_v4u *>(g);
            lds[p[0] * t.pitch + f[0]] = v.x; lds[p[1] * t.pitch + f[1]] = v.y;
            lds[p[2] * t.pitch + f[2]] = v.z; lds[p[3] * t.pitch + f[3]] = v.w;
        } else {
            planes_v4u v;
            v.x = lds[p[0] * t.pitch + f[0]]; v.y = lds[p[1] * t.pitch + f[1]];
            v.z = lds[p[2] * t.pitch + f[2]]; v.w = lds[p[3] * t.pitch + f[3]];
            planes_st4<NT>(g, v);
        }
    }
    for (int i = nv + tid; i < n; i += 256) {
        const int f = (int)__umulhi((unsigned)i, m), p = i - f * t.tp;
        uint32_t *g = rows + (t.f0 + f) * NP + t.p0 + p;
        if constexpr (TO_LDS) lds[p * t.pitch + f] = *g;
        else planes_st1<NT>(g, lds[p * t.pitch + f]);
    }
}

// plane side: plane p0 + p, frames f0 .. f0 + tf - 1 at planes[(p0 + p) * stride + f0 + f]
template <bool TO_LDS, bool NT>
__device__ __forceinline__ void planes_plane_side(uint32_t *planes, long stride, const PlanesTile &t, uint32_t *lds, bool vec)
{
    const int tid = threadIdx.x;
    if (vec) {
        const int TQ = t.TF / 4, nq = t.tp * TQ; // quads of a full tile, plane by plane
        const unsigned m = planes_magic((unsigned)TQ);
        for (int j = tid; j < nq; j += 256) {
            const int p = (int)__umulhi((unsigned)j, m), f = 4 * (j - p * TQ);
            if (f >= t.tf) continue;
            uint32_t *g = planes + (long)(t.p0 + p) * stride + t.f0 + f;
            uint32_t *l = lds + p * t.pitch + f;
            if (f + 3 < t.tf) {
                if constexpr (TO_LDS) {
                    const planes_v4u v = *reinterpret_cast<const planes_v4u *>(g);
                    l[0] = v.x; l[1] = v.y; l[2] = v.z; l[3] = v.w;
                } else planes_st4<NT>(g, planes_v4u{l[0], l[1], l[2], l[3]});
            } else { // the quad the end of the message cuts
                for (int k = 0; f + k < t.tf; ++k) {
                    if constexpr (TO_LDS) l[k] = g[k];
                    else planes_st1<NT>(g + k, l[k]);
                }
            }
        }
    } else {
        const int n = t.tp * t.TF;
        const unsigned m = planes_magic((unsigned)t.TF);
        for (int j = tid; j < n; j += 256) {
            const int p = (int)__umulhi((unsigned)j, m), f = j - p * t.TF;
            if (f >= t.tf) continue;
            uint32_t *g = planes + (long)(t.p0 + p) * stride + t.f0 + f;
            if constexpr (TO_LDS) lds[p * t.pitch + f] = *g;
            else planes_st1<NT>(g, lds[p * t.pitch + f]);
        }
    }
}

// grid: x = tiles of TF frames, y = chunks of 64 planes
template <bool TO_PLANES, bool NT>
__global__ __launch_bounds__(256) void planes_kernel(uint32_t *rows, uint32_t *planes, long nrows, int NP, long stride, int TF, int row_vec,
                                                     int plane_vec)
{
    __shared__ uint32_t lds[PLANES_LDS];
    PlanesTile t;
    t.TF = TF;
    t.pitch = TF + 1;
    t.p0 = (int)blockIdx.y * PLANES_TP;
    t.tp = NP - t.p0 < PLANES_TP ? NP - t.p0 : PLANES_TP;
    t.f0 = (long)blockIdx.x * TF;
    t.tf = nrows - t.f0 < TF ? (int)(nrows - t.f0) : TF;
    if (TO_PLANES) planes_row_side<true, false>(rows, NP, t, lds, row_vec != 0);
    else planes_plane_side<true, false>(planes, stride, t, lds, plane_vec != 0);
    __syncthreads();
    if (TO_PLANES) planes_plane_side<false, NT>(planes, stride, t, lds, plane_vec != 0);
    else planes_row_side<false, NT>(rows, NP, t, lds, row_vec != 0);
}

} // namespace redio
using namespace redio;


constexpr size_t PLANES_NT_BYTES = (size_t)256 << 20; // the last-level cache: a larger message is not there when its consumer starts

static int planes_launch(bool to_planes, const void *d_rows, const void *d_planes, size_t nrows, int nchan, size_t plane_stride, void *stream)
{
    if (nchan < 1 || plane_stride < nrows) return REDIO_ERR_ARG;
    if (nrows == 0) return REDIO_OK;
    if (!d_rows || !d_planes || ((uintptr_t)d_rows & 3) || ((uintptr_t)d_planes & 3)) return REDIO_ERR_ARG;
    if (nchan > (1 << 20)) return REDIO_ERR_UNSUPPORTED; // 65535 chunks of 64 planes in a grid
    const int NP = 2 * nchan, tp_full = NP < PLANES_TP ? NP : PLANES_TP, TF = planes_tile_frames(tp_full);
    const int row_vec = ((uintptr_t)d_rows & 15) == 0 && (NP <= PLANES_TP || NP % 4 == 0);
    const int plane_vec = ((uintptr_t)d_planes & 15) == 0 && plane_stride % 4 == 0;
    const bool nt = nrows * (size_t)NP * sizeof(float) >= PLANES_NT_BYTES;
    auto kern = to_planes ? (nt ? planes_kernel<true, true> : planes_kernel<true, false>) : (nt ? planes_kernel<false, true> : planes_kernel<false, false>);
    // HIP rejects a launch of 2^32 threads or more: at most 2^24 - 1 workgroups per launch, whole tiles each (the bases of a later launch
    // keep the alignment of the first: a tile is a multiple of 64 frames)
    const size_t gy = (size_t)(NP + PLANES_TP - 1) / PLANES_TP, tiles = (nrows + (size_t)TF - 1) / (size_t)TF, per_launch = 0xffffffu / gy;
    for (size_t t0 = 0; t0 < tiles; t0 += per_launch) {
        const size_t nt_tiles = tiles - t0 < per_launch ? tiles - t0 : per_launch, f0 = t0 * (size_t)TF;
        const size_t frames = nrows - f0 < nt_tiles * (size_t)TF ? nrows - f0 : nt_tiles * (size_t)TF;
        hipLaunchKernelGGL(kern, dim3((unsigned)nt_tiles, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, (uint32_t *)d_rows + f0 * (size_t)NP,
                           (uint32_t *)d_planes + f0, (long)frames, NP, (long)plane_stride, TF, row_vec, plane_vec);
    }
    return hip_rc(hipGetLastError());
}

extern "C" int redio_rows_to_planes_c32(const void *d_rows, size_t nrows, int nchan, void *d_planes, size_t plane_stride, void *stream)
{
    return planes_launch(true, d_rows, d_planes, nrows, nchan, plane_stride, stream);
}

extern "C" int redio_planes_to_rows_c32(const void *d_planes, size_t plane_stride, size_t nrows, int nchan, void *d_rows, void *stream)
{
    return planes_launch(false, d_rows, d_planes, nrows, nchan, plane_stride, stream);
}
