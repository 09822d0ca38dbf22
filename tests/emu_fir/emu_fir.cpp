// emu_fir.cpp -- CPU emulation of the FIR's chunked tiled kernel (libredio_amd/csrc/fir_tile_kernels.h, fir_chunked_kernel with the plain
// loader): every thread of one workgroup runs tile_load_thread into the padded image, fir_chunks on it, the transpose and the store
// loop -- the very sources the device compiles (fir_tile.h, fir_chunks.h), in the kernel's order, one barrier's phase after the other.
// The image has exactly tile_lds_elems elements between two fences of NaN: a write outside is counted and never performed, a lane
// program that reads outside computes NaN.
#include "../../libredio_amd/csrc/fir_chunks.h"
#include "../../libredio_amd/csrc/fir_tile.h"
#include <cmath>
#include <vector>

using namespace redio;

namespace {
constexpr long FENCE = 8192;

// the LDS allocation as the kernel indexes it: xs[i]
template <typename T>
struct Image {
    std::vector<T> all; long elems; int bad = 0; T sink{};
    explicit Image(long n) : all((size_t)(n + 2 * FENCE)), elems(n) { for (T &v : all) v = nan_of(); }
    static T nan_of() { if constexpr (sizeof(T) == 8) return T{NAN, NAN}; else return NAN; }
    T *data() { return all.data() + FENCE; }
    T &operator[](long i) { if (i < 0 || i >= elems) { ++bad; return sink; } return data()[i]; }
};

struct Call {
    int K; const void *x; long n_in; const float *taps; long tile; void *y; long n_out;
};

template <typename T, bool FUSED, int D>
int tile(const Call &c)
{
    constexpr int NT = 256, R = tile_r(D), CHW = tile_chw(D), TILE_OUT = NT * R, LSTR = R * D, VEC = 16 / (int)sizeof(T);
    constexpr bool STREAM = D >= 2;
    const long elems = tile_lds_elems(R, D, tile_window(c.K));
    if (elems * (long)sizeof(T) > TILE_LDS_MAX) return -1; // launch_chunked: not this kernel's
    const T *x = static_cast<const T *>(c.x);
    T *y = static_cast<T *>(c.y);
    const bool vec_in = ((uintptr_t)x & 15) == 0, vec_out = ((uintptr_t)y & 15) == 0;
    Image<T> xs(elems);
    const long in0 = c.tile * TILE_OUT * D;
    for (int tid = 0; tid < NT; ++tid)
        tile_load_thread<T, STREAM, 8>(tid, NT, x + in0, c.n_in - in0, (int)tile_in(R, D, tile_window(c.K)), vec_in, [&](int n, auto v) {
            const long d = tile_image_index(n, LSTR); // the kernel's sink: the samples of one load side by side
            if constexpr (std::is_same_v<decltype(v), float4>)
                for (int e = 0; e < VEC; ++e) xs[d + e] = tile_elem<T>(v, e);
            else xs[d] = v;
        });
    std::vector<T> acc((size_t)TILE_OUT);
    for (int tid = 0; tid < NT; ++tid) {
        T a[R];
        for (int r = 0; r < R; ++r) a[r] = T{};
        fir_chunks<T, D, R, FUSED, CHW>(xs.data(), tile_lane_base(tid, LSTR), c.K, c.taps, a);
        for (int r = 0; r < R; ++r) acc[(size_t)tid * R + r] = a[r];
    }
    for (int tid = 0; tid < NT; ++tid) {
        T a[R];
        for (int r = 0; r < R; ++r) a[r] = acc[(size_t)tid * R + r];
        tile_transpose_put<T, R>(xs, tid, a);
    }
    const long o0 = c.tile * TILE_OUT;
    for (int tid = 0; tid < NT; ++tid)
        tile_store_thread<T, STREAM>(tid, NT, xs, TILE_OUT, y + o0, c.n_out - o0, vec_out, [](int e) { return tile_transpose_index(e, R); });
    return xs.bad;
}

// the fold, written out: ascending taps, a rounded multiply then a rounded add, or fmaf
template <bool FUSED>
float fold1(const float *x, long stride, const float *h, int K)
{
    float acc = 0.0f;
    for (int j = 0; j < K; ++j) acc = FUSED ? fmaf(x[j * stride], h[j], acc) : acc + x[j * stride] * h[j];
    return acc;
}
} // namespace

extern "C" {

// the table and the allocation as the headers have them; 0 where the decimation has no chunked form
int emu_fir_r(long D) { return tile_r(D); }
int emu_fir_chw(long D) { return tile_chw(D); }
long emu_fir_lds_elems(long K, long D) { return tile_r(D) ? tile_lds_elems(tile_r(D), D, tile_window(K)) : 0; }
long emu_fir_lds_max(void) { return TILE_LDS_MAX; }

// Workgroup `tile` of the chunked kernel on n_in samples at x (f32, or cf32 with cplx; any whole-sample alignment, as y): writes the
// tile's share of the n_out outputs to y.  taps: K floats, zero-padded to a multiple of 16.  Returns the count of image writes outside
// the allocation, -1 where the launcher would refuse the shape (no chunked form, or beyond the LDS budget).
int emu_fir_tile(int cplx, int fused, long D, int K, const void *x, long n_in, const float *taps, long tile_no, void *y, long n_out)
{
    const Call c = {K, x, n_in, taps, tile_no, y, n_out};
    return tile_dispatch_d(D, -1, [&](auto d) {
        constexpr int DD = decltype(d)::value;
        if (cplx) return fused ? tile<float2, true, DD>(c) : tile<float2, false, DD>(c);
        return fused ? tile<float, true, DD>(c) : tile<float, false, DD>(c);
    });
}

// y[i] = the fold over x[i D + j] h[j] for i < n_out, each component of a complex sample on its own
void emu_fir_fold(int cplx, int fused, long D, int K, const float *x, const float *h, float *y, long n_out)
{
    const long c = cplx ? 2 : 1;
    for (long i = 0; i < n_out; ++i)
        for (long p = 0; p < c; ++p)
            y[i * c + p] = fused ? fold1<true>(x + i * D * c + p, c, h, K) : fold1<false>(x + i * D * c + p, c, h, K);
}
}
