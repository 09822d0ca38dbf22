// The part of the polyphase spectrometer's workgroup kernel (libredio_amd/csrc/pfb_pspec_p2.hip, pfbspec_p2_kernel) that lies behind
// the channelizer's transform, run on the CPU: every thread of every workgroup, one at a time, with the launcher's stream geometry
// and the fold of pfb_pspec_p2_core.h -- the workgroup's iteration count, the powers of the thread's own channels of its stream's rows,
// the fold state machine and the stores of finished units.  The image behind the transform holds bin n of the stream's row tb + ti;
// here those are the channelizer's rows as the oracle computed them, clamped behind the call's last row as the kernel's loads are.
#include "../../libredio_amd/csrc/pfb_pspec_p2_core.h"
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

// One launch.  rows: the channelizer's rows [nrows_total][M]; pair: the load form (two neighbouring channels per thread and load;
// 512 and 1024 channels only); nunits units (output rows, or with `split` segments); ups: units per stream, 0 for the launcher's own
// choice on a device of `cus` CUs.  dst: M f32 per unit; stores: writes per element of dst; owners: streams per unit;
// stream_rows: [t0, t1) per stream slot of the grid; group_iters: the iteration count each workgroup runs.
// Returns the workgroup count, or -1 if the shape's constants disagree with pfb_pspec_p2_core.h, -2 if an array is too short.
extern "C" long emu_pfbspec_p2(const float2 *rows, long nrows_total, int M, int pair, long K, int split, long nunits, long ups, long cus, float *dst,
                               int *stores, int *owners, long *stream_rows, long *group_iters, long max_groups)
{
    // pfbspec_p2_kernel's shape constants
    const int NP = pair ? (M <= 512 ? 1 : M / 512) : (M <= 256 ? 1 : M / 256);
    const int CPT = pair ? 2 * NP : NP, MT = M / CPT, G = 256 / MT, TR = 16 / CPT;
    if (G != pfbspec_p2_streams_per_group(M) || TR != pfbspec_p2_rows_per_iter(M) || G * TR * M != 4096) return -1;
    auto chan = [&](int m, int c) { return pair ? 2 * m + (c & 1) + 512 * (c >> 1) : m + 256 * c; };
    if (ups <= 0) ups = pfbspec_p2_units_per_stream(nunits, K, split != 0, cus, M);
    const long nstreams = (nunits + ups - 1) / ups, grid = (nstreams + G - 1) / G;
    if (grid > max_groups) return -2;
    const Counted out{dst, stores};
    for (long b = 0; b < grid; ++b) {
        // the exchange of the iteration counts: thread (0, g) writes its stream's, every thread takes the maximum
        long iters = 0;
        for (int g = 0; g < G; ++g) {
            const PfbSpecP2Stream st = pfbspec_p2_stream(b * G + g, ups, nunits, nrows_total, K, split != 0);
            const long n = pfbspec_p2_stream_iters(st, TR);
            iters = n > iters ? n : iters;
            stream_rows[2 * (b * G + g)] = st.t0; stream_rows[2 * (b * G + g) + 1] = st.t1;
            for (long u = st.u0; u < st.u1; ++u) ++owners[u];
        }
        group_iters[b] = iters;
        for (int tid = 0; tid < 256; ++tid) {
            const int m = tid % MT, g = tid / MT;
            const PfbSpecP2Stream st = pfbspec_p2_stream(b * G + g, ups, nunits, nrows_total, K, split != 0);
            PfbSpecFold fold;
            long tf;
            pfbspec_fold_begin(fold, st.u0, K, split != 0, tf);
            std::vector<float> seg(CPT, 0.f), row(CPT, 0.f), pw(CPT);
            for (long it = 0; it < iters; ++it) {
                const long tb = st.t0 + (long)TR * it;
                for (int ti = 0; ti < TR; ++ti) {
                    long r = tb + ti;
                    r = r < nrows_total ? r : nrows_total - 1; // computed from clamped loads, never summed
                    for (int c = 0; c < CPT; ++c) pw[c] = pspec_power(rows[r * M + chan(m, c)]);
                    if (tb + ti < st.t1) {
                        const PspecStep ps = pspec_step(fold.i, fold.cnt);
                        for (int c = 0; c < CPT; ++c) pfbspec_p2_fold_accum(ps, pw[c], seg[c], row[c]);
                        if (pfbspec_p2_fold_ends(fold))
                            for (int c = 0; c < CPT; ++c) out[fold.u * M + chan(m, c)] = row[c];
                        pfbspec_p2_fold_next(fold, K, split != 0);
                    }
                }
            }
        }
    }
    return grid;
}

// the launcher's own numbers, for the tests' restatement of them
extern "C" long emu_pfbspec_p2_units_per_stream(long nunits, long K, int split, long cus, int M) { return pfbspec_p2_units_per_stream(nunits, K, split != 0, cus, M); }
extern "C" long emu_pfbspec_p2_split_rows(long K, long cus, int M) { return pfbspec_p2_split_rows(K, cus, M); }
extern "C" int emu_pfbspec_p2_streams_per_group(int M) { return pfbspec_p2_streams_per_group(M); }
extern "C" int emu_pfbspec_p2_rows_per_iter(int M) { return pfbspec_p2_rows_per_iter(M); }
// {u0, u1, t0, t1} of stream s
extern "C" void emu_pfbspec_p2_stream(long s, long ups, long nunits, long rows, long K, int split, long *out)
{
    const PfbSpecP2Stream st = pfbspec_p2_stream(s, ups, nunits, rows, K, split != 0);
    out[0] = st.u0; out[1] = st.u1; out[2] = st.t0; out[3] = st.t1;
}
