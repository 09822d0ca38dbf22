// The part of the fused polyphase spectrometer (libredio_amd/csrc/pfb_pspec_kernels.hip, pfbspec64_kernel) that lies behind the
// channelizer's transform, run on the CPU: sixty-four lanes one at a time in the kernel's own phases -- the power tile's stores,
// its loads, the fold state machine and the stores of finished units (pfb_pspec_core.h).  A phase ends where the kernel has a
// wave_lds_fence().  The channelizer's rows come in as the oracle computed them, dealt to the lanes as pfb_fft64_passC leaves them.
#include "../../libredio_amd/csrc/pfb_pspec_core.h"
#include <vector>

using namespace redio;

namespace {
// a destination that counts the writes each element receives
struct Counted {
    float *p;
    int *n;
    struct Ref {
        float *q;
        int *c;
        void operator=(float v) const { *q = v; ++*c; }
    };
    Ref operator[](long i) const { return Ref{p + i, n + i}; }
};
} // namespace

// One launch: rows = the channelizer's rows [nrows_total][64]; nunits units (output rows, or with `split` segments), units_per_wave
// per wavefront (0: the launcher's own choice); dst: 64 f32 per unit; stores: writes per element of dst.  Returns the wave count.
extern "C" long emu_pfbspec(const float2 *rows, long nrows_total, long K, int split, long nunits, long units_per_wave, float *dst, int *stores)
{
    if (units_per_wave <= 0) units_per_wave = pfbspec_units_per_wave(nunits, K, split != 0);
    const Counted out{dst, stores};
    long nwaves = 0;
    std::vector<float> tile(PFBSPEC_LDS);
    for (long u0 = 0; u0 < nunits; u0 += units_per_wave, ++nwaves) {
        const long u1 = u0 + units_per_wave < nunits ? u0 + units_per_wave : nunits;
        PfbSpecFold fold[64];
        long t0 = 0;
        for (int lane = 0; lane < 64; ++lane) pfbspec_fold_begin(fold[lane], u0, K, split != 0, t0);
        const long t1 = pfbspec_units_end(u1, K, split != 0);
        float seg[64], row[64];
        for (int lane = 0; lane < 64; ++lane) seg[lane] = row[lane] = 0.f;
        for (long tb = t0; tb < t1; tb += PFB_TILE) {
            for (int lane = 0; lane < 64; ++lane) { // after pass C: w[k0 + 4 k2] = X[pfb_out_channel(lane, k0, k2)] of row tb + (lane >> 2)
                long r = tb + (lane >> 2);
                r = r < nrows_total ? r : nrows_total - 1; // rows behind the wave's last are computed from clamped loads and never summed
                float2 w[16];
                for (int k0 = 0; k0 < 4; ++k0)
                    for (int k2 = 0; k2 < 4; ++k2) w[k0 + 4 * k2] = rows[r * PFB_M + pfb_out_channel(lane, k0, k2)];
                for (int k0 = 0; k0 < 4; ++k0) {
                    const float4 p = pfbspec_power4(w, k0);
                    float *q = tile.data() + pfbspec_tile_index(lane >> 2, pfb_out_channel(lane, k0, 0));
                    q[0] = p.x; q[1] = p.y; q[2] = p.z; q[3] = p.w;
                }
            }
            for (int lane = 0; lane < 64; ++lane) {
                float pw[PFB_TILE];
                for (int tt = 0; tt < PFB_TILE; ++tt) pw[tt] = tile[pfbspec_tile_index(tt, lane)];
                for (int tt = 0; tt < PFB_TILE; ++tt)
                    if (tb + tt < t1) pfbspec_fold_step(fold[lane], pw[tt], seg[lane], row[lane], K, split != 0, out, lane);
            }
        }
    }
    return nwaves;
}
