// emu_ddc.cpp -- CPU emulation of the tuner's kernels (the FIR's tiled bodies with the loader of ddc_core.h): every thread of one workgroup
// runs that loader into the padded LDS image (fir_tile.h), then the FIR lane program (fir_core.h fir_lane, fir_chunks.h fir_chunks) runs on that image --
// the very sources the device compiles.  Also the counters of one carried-history call (stream_split.h) with the tuner's phase.
#include "../../libredio_amd/csrc/ddc_core.h"
#include "../../libredio_amd/csrc/fir_chunks.h"
#include "../../libredio_amd/csrc/stream_split.h"
#include <cmath>
#include <vector>

using namespace redio;

namespace {
struct Call {
    int K; long D; bool u8, fused; const char *x; long n_in; unsigned long long first; const float2 *tab; unsigned L; const float *taps; long tile; bool vec_x;
    float2 *image, *y; int *tile_in, *tile_out, *bad;
};

// the LDS image: exactly `elems` elements between two fences of NaN, FENCE elements each.  A write outside [0, elems) is counted, never
// performed; a lane program that reads outside computes NaN from the fence
constexpr long FENCE = 8192;
struct Image {
    std::vector<float2> all; long elems; int *bad;
    Image(long n, int *b) : all((size_t)(n + 2 * FENCE), make_float2(NAN, NAN)), elems(n), bad(b) {}
    float2 *data() { return all.data() + FENCE; }
    float2 at(long i) { return data()[i]; }
    void put(long i, float2 v) { if (i < 0 || i >= elems) ++*bad; else data()[i] = v; }
};

template <bool U8, bool STREAM, typename Index>
void load(const Call &c, long in0, int tile_in, Image &im, Index index)
{
    const unsigned base = ddc_base(ddc_first_mod(c.first, c.L), (unsigned long long)in0, c.L);
    for (int tid = 0; tid < 256; ++tid)
        ddc_load_thread<U8, STREAM>(tid, 256, c.x + in0 * (U8 ? 2 : 8), c.n_in - in0, c.tab + base, tile_in, c.vec_x, (base & 1u) == 0,
                                    [&](int n, float2 v) { im.put(index(n), v); });
}

template <bool U8, bool FUSED, int K, int D, int R>
void tiled(const Call &c)
{
    using G = FirGeom<K, D, R>;
    constexpr int TILE_OUT = 256 * R, TILE_IN = G::tile_in(TILE_OUT);
    Image im(G::lds_elems(TILE_OUT), c.bad);
    load<U8, false>(c, c.tile * TILE_OUT * D, TILE_IN, im, [](int n) { return (long)G::lds_index(n); });
    for (int n = 0; n < TILE_IN; ++n) c.image[n] = im.at(G::lds_index(n));
    *c.tile_in = TILE_IN; *c.tile_out = TILE_OUT;
    if (!c.y) return;
    for (int tid = 0; tid < 256; ++tid) {
        float2 acc[R];
        for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);
        fir_lane<float2, K, D, R, FUSED>(im.data(), tid, c.taps, acc);
        for (int r = 0; r < R; ++r) c.y[tid * R + r] = acc[r];
    }
}

template <bool U8, bool FUSED, int D>
void chunked(const Call &c)
{
    constexpr int R = tile_r(D), CHW = tile_chw(D), LSTR = R * D, TILE_OUT = 256 * R;
    const int tile_in = (int)redio::tile_in(R, D, tile_window(c.K));
    Image im(tile_lds_elems(R, D, tile_window(c.K)), c.bad);
    load<U8, (D >= 2)>(c, c.tile * TILE_OUT * D, tile_in, im, [](int n) { return (long)tile_image_index(n, LSTR); });
    for (int n = 0; n < tile_in; ++n) c.image[n] = im.at(tile_image_index(n, LSTR));
    *c.tile_in = tile_in; *c.tile_out = TILE_OUT;
    if (!c.y) return;
    for (int tid = 0; tid < 256; ++tid) {
        float2 acc[R];
        for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);
        fir_chunks<float2, D, R, FUSED, CHW>(im.data(), tile_lane_base(tid, LSTR), c.K, c.taps, acc);
        for (int r = 0; r < R; ++r) c.y[tid * R + r] = acc[r];
    }
}

template <bool U8, bool FUSED>
void direct(const Call &c)
{
    const long n_out = c.n_in < c.K ? 0 : (c.n_in - c.K) / c.D + 1;
    *c.tile_in = 0; *c.tile_out = 256;
    if (!c.y) return;
    for (int tid = 0; tid < 256; ++tid) {
        const long i = c.tile * 256 + tid;
        if (i >= n_out) { c.y[tid] = make_float2(0.f, 0.f); continue; }
        const unsigned idx0 = ddc_base(ddc_first_mod(c.first, c.L), (unsigned long long)(i * c.D), c.L);
        c.y[tid] = ddc_direct_output<U8, FUSED>(c.x + i * c.D * (U8 ? 2 : 8), idx0, c.tab, c.L, c.taps, c.K);
    }
}

template <bool U8, bool FUSED>
int run(const Call &c)
{
    const int route = ddc_route(c.K, c.D);
    if (route == 1) {
        if (c.K == 127 && c.D == 5) tiled<U8, FUSED, 127, 5, 4>(c);
        else if (c.K == 127 && c.D == 1) tiled<U8, FUSED, 127, 1, 8>(c);
        else if (c.K == 63 && c.D == 1) tiled<U8, FUSED, 63, 1, 8>(c);
        else tiled<U8, FUSED, 63, 5, 4>(c);
    } else if (route == 2) {
        tile_dispatch_d(c.D, 0, [&](auto d) { chunked<U8, FUSED, decltype(d)::value>(c); return 0; });
    } else {
        direct<U8, FUSED>(c);
    }
    return route;
}
} // namespace

extern "C" {

int emu_ddc_table_ext(void) { return DDC_TABLE_EXT; }
int emu_ddc_route(long K, long D) { return ddc_route(K, D); }
// the chunked route's geometry as the headers have it; 0 where the decimation has no chunked form
long emu_ddc_chunked_tile_in(long K, long D) { return tile_r(D) ? tile_in(tile_r(D), D, tile_window(K)) : 0; }
long emu_ddc_chunked_lds_elems(long K, long D) { return tile_r(D) ? tile_lds_elems(tile_r(D), D, tile_window(K)) : 0; }
int emu_ddc_chunked_chw(long D) { return tile_chw(D); }

// One workgroup (`tile`) of a call on n_in samples at x (cf32, or u8 I/Q bytes), first_index `first`.  tab: the device table's layout,
// L + emu_ddc_table_ext() entries (the caller may append a fence behind it).  image: the tile's samples as the lane program sees them, in
// tile order (read back through the image's index map; NaN where the loader wrote nothing); y: the workgroup's outputs, zero-filled
// samples included; y == NULL runs the loader alone.  *bad counts image writes outside the allocation.  Returns the route.
int emu_ddc_tile(int K, long D, int u8, int fused, const void *x, long n_in, unsigned long long first, const float *tab, unsigned L, const float *taps,
                 long tile, int vec_x, float *image, float *y, int *tile_in, int *tile_out, int *bad)
{
    const Call c = {K, D, u8 != 0, fused != 0, (const char *)x, n_in, first, (const float2 *)tab, L, taps, tile, vec_x != 0,
                    (float2 *)image, (float2 *)y, tile_in, tile_out, bad};
    *bad = 0;
    if (u8) return fused ? run<true, true>(c) : run<true, false>(c);
    return fused ? run<false, true>(c) : run<false, false>(c);
}

// The counters of one carried-history call of n new samples (stream_carry.hip carry_enqueue): state = {hist, skip, total_in, total_units},
// out = {nh, the head's first_index, nb, the body's first_index}
void emu_ddc_stream_step(unsigned long long *state, size_t W, size_t H, size_t n, unsigned long long *out)
{
    size_t hist = (size_t)state[0], skip = (size_t)state[1];
    const size_t n_call = n, drop = skip < n ? skip : n;
    n -= drop;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (n == 0) { state[1] = skip - drop; state[2] += n_call; return; }
    const StreamSplit s = stream_split(hist, W, H, n);
    out[0] = s.nh; out[1] = stream_head_first(state[2], hist); out[2] = s.nb; out[3] = stream_body_first(state[2], drop, s);
    const size_t consumed = (s.nh + s.nb) * H;
    if (consumed >= hist + n) { state[0] = 0; state[1] = consumed - (hist + n); }
    else { state[0] = hist + n - consumed; state[1] = skip - drop; }
    state[2] += n_call;
    state[3] += s.nh + s.nb;
}
}
