// fir_chunks.h -- the chunked lane program of the any-taps tiled FIR kernel (fir_tile_kernels.h), which the tuner instantiates with its
// own loader on the same padded LDS image (fir_tile.h).  Host-compilable (tests/emu_fir, tests/emu_ddc): the device-only window reads
// are behind __HIP_DEVICE_COMPILE__.
#pragma once
#include "fir_core.h"

namespace redio {

// ---- chunked tiled kernel: ANY tap count, decimation from a small compile-time set ---------------
// The register blocking of fir_core.h needs compile-time tap indices; here the taps are walked in chunks of
// CH = 16 with a run-time chunk count instead: per chunk a lane reads the CH + (R-1)*D samples its R outputs
// need for these taps (statically indexed registers), the 16 taps arrive as one scalar load, and the
// multiply-adds are fully unrolled inside the chunk.  Every accumulator still receives its products in
// ascending tap order (chunks ascending, taps ascending inside a chunk), so results are bit-identical to the
// reference fold.  The K % 16 taps behind the last whole chunk run as chunks of 8, 4, 2 and 1 taps (the binary
// digits of the remainder): the same straight-line code at smaller sizes, no per-tap guard (a guarded 16-tap
// chunk compiled to a select per product and cost as much as three whole chunks).
// ALIGNED: j0 is a multiple of the lane stride R*D (whole chunks whose size is one), so the pad element count of window sample i
// is j0 / LSTR + i / LSTR with a compile-time second term: one scalar base per chunk and immediate offsets.  Round 3: before, every
// one of the window reads paid a wave-uniform division by LSTR (SQ counters of 255 taps / 10: 9.0e7 scalar against 6.7e7 vector
// instructions per launch).
template <typename T, int D, int R, bool FUSED, int CH, bool ALIGNED = false>
RD_D void fir_chunk(const T *xs, int base, int j0, const float *__restrict__ taps, T (&acc)[R])
{
    constexpr int WIN = CH + (R - 1) * D, LSTR = R * D;
    constexpr bool PAD = (LSTR % 2) == 0;
    T xv[WIN];
    const int cb = base + (PAD ? j0 + j0 / LSTR : j0); // ALIGNED: the window's first sample in the image
    float h[CH];
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (ALIGNED && sizeof(T) == 8) {
        // One ds_read_b64 per sample, spelled out: from base + immediate the compiler pairs them into ds_read2_b64, which the LDS
        // serves at half the bytes per clock (MI355X_MICROARCH.md, LDS table: 8 cycles against 2 x 2; SQ_LDS_IDX_ACTIVE of this
        // kernel rose by half when the offsets became immediates).  The reads land in order behind the taps' scalar load.
        typedef float v2f __attribute__((ext_vector_type(2)));
        v2f q[WIN];
        const unsigned a = (unsigned)(unsigned long long)(const __attribute__((address_space(3))) void *)(xs + cb);
#pragma unroll
        for (int i = 0; i < WIN; ++i) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(q[i]) : "v"(a), "n"((PAD ? i + i / LSTR : i) * 8));
#pragma unroll
        for (int j = 0; j < CH; ++j) h[j] = taps[j0 + j];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
            asm volatile("" : "+v"(q[i])); // uses stay behind the wait
            xv[i] = T{q[i].x, q[i].y};
        }
    } else
#endif
    {
#pragma unroll
        for (int i = 0; i < WIN; ++i) {
            const int m = j0 + i; // wave-uniform
            xv[i] = ALIGNED ? xs[cb + (PAD ? i + i / LSTR : i)] : xs[base + (PAD ? m + m / LSTR : m)];
        }
#pragma unroll
        for (int j = 0; j < CH; ++j) h[j] = taps[j0 + j];
    }
#pragma unroll
    for (int i = 0; i < WIN; ++i)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int j = i - r * D;
            if (j >= 0 && j < CH) acc[r] = mac<FUSED>(xv[i], h[j], acc[r]);
        }
}

// A two-stage form of the whole chunks (window reads and taps of chunk c + 1 in flight into a second register set during the
// multiply-adds of chunk c, chunks of one lane stride) was built and measured slower on all ten shapes tried (255 taps / 10: 0.192 ms
// against 0.178; 101 / 3: 0.188 against 0.154): 100-190 VGPRs instead of 50-110, and the occupancy they cost hid more latency than
// the second register set did.  profiles/r03_fir_chunked.txt.
// all K taps of the R outputs of a lane: whole chunks, then the remainder's binary digits
template <typename T, int D, int R, bool FUSED, int CH = 16>
RD_D void fir_chunks(const T *xs, int base, int K, const float *__restrict__ taps, T (&acc)[R])
{
    constexpr bool ALIGNED = CH % (R * D) == 0;
    const int nfull = K / CH;
    for (int c = 0; c < nfull; ++c) fir_chunk<T, D, R, FUSED, CH, ALIGNED>(xs, base, c * CH, taps, acc);
    int j0 = nfull * CH;
    const int rest = K - j0; // < CH: its binary digits as chunks of 32, 16, 8, 4, 2, 1 taps
    if (CH > 32 && (rest & 32)) { fir_chunk<T, D, R, FUSED, 32>(xs, base, j0, taps, acc); j0 += 32; }
    if (CH > 16 && (rest & 16)) { fir_chunk<T, D, R, FUSED, 16>(xs, base, j0, taps, acc); j0 += 16; }
    if (rest & 8) { fir_chunk<T, D, R, FUSED, 8>(xs, base, j0, taps, acc); j0 += 8; }
    if (rest & 4) { fir_chunk<T, D, R, FUSED, 4>(xs, base, j0, taps, acc); j0 += 4; }
    if (rest & 2) { fir_chunk<T, D, R, FUSED, 2>(xs, base, j0, taps, acc); j0 += 2; }
    if (rest & 1) fir_chunk<T, D, R, FUSED, 1>(xs, base, j0, taps, acc);
}

} // namespace redio
