// chain_v4.hip -- the north-star chain kernel: one wavefront per run of consecutive 1024-sample decimated blocks.
//   * a wave owns a CONTIGUOUS range of blocks, so consecutive sub-tiles (256 outputs) are consecutive in the stream;
//   * the 122-sample FIR halo that two consecutive sub-tiles share is carried over inside the CU
//     (one 16-byte LDS read + write per lane) instead of being fetched again: per sub-tile exactly
//     640 x 16 B = 10 loads per lane of NEW samples;
//   * the FIR results stay in registers in the operand layout of the one-wave 1024-point transform.
// Bit-exact with the oracle (FIR fold order of dsputils.rs:30-32, kissfft butterfly order).
#ifndef REDIO_EXP_CHAIN_NT
#define REDIO_EXP_CHAIN_NT 3 // bit 0: non-temporal stream loads, bit 1: non-temporal spectrum stores (fft_wave.h)
#endif
// The seam between two sub-tiles and the wave's prologue (round 12, profiles/r12_chain_seam.txt), one bit per item so that the
// measurement build can time each on its own (tools/chain_seam_ab.sh); a bit that is clear builds the parent's code for that item:
//   bit 0  lane-constant LDS addresses (window base, halo slots, park slots, the transform's exchange rows) computed once per wave
//   bit 1  stream loads and output stores through buffer descriptors of the wave's own run: scalar base, one constant lane offset
//   bit 2  the halo's LDS read under the FIR's last chunk, its write branch-free behind the last window read
//   bit 3  prologue: every request (taps, head, first sub-tile, twiddles) issued before the first wait
#ifndef REDIO_EXP_SEAM
#define REDIO_EXP_SEAM 15
#endif
#include "fir_core.h"
#include "fft_wave.h"
#include "redio_internal.h"
#include "../../include/redio.h"
#include <type_traits>

namespace redio {

typedef float v4f_t __attribute__((ext_vector_type(4)));

constexpr int chain_gcd(int a, int b) { return b == 0 ? a : chain_gcd(b, a % b); }

template <int N, typename F>
__device__ __forceinline__ void static_for4(F &&f)
{
    if constexpr (N > 0) {
        static_for4<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// FIR_ONLY: the same data movement and FIR, but the decimated samples are stored instead of transformed
// (the stand-alone decimating FIR of redio_fir_* for this shape); `out` then holds 1024 outputs per block.
// IN_U8: `x` is the receiver's own format, interleaved u8 I/Q bytes (rtlsdr::data_to_samples, rtlsdr.rs:159-162: i as f32 / 127.0 - 1.0):
// a lane's 16-byte load of two cf32 samples becomes a 4-byte load of the same two samples, converted on the way into the LDS image --
// 2 + 1.6 bytes per sample through HBM instead of 8 + 8 + 1.6 for the conversion kernel followed by this one.
// PF2: TWO sub-tiles of loads in flight (round 6): a second register set of NLD pairs, the loop unrolled by two with the
// roles of the sets swapped -- the request for sub-tile j + 2 is issued before the FIR of sub-tile j, the set holding j + 1 is parked behind it.
// RES: the FIR runs with the taps resident in scalar registers (fir_lane_v_res).  PRECONDITION of RES: the taps are bit-palindromic
// (taps[i] and taps[K-1-i] the same 32-bit pattern); the host decides that once per plan (taps_bit_palindromic) and every launcher
// below takes the answer.  !RES: any taps (fir_lane_v, staged per chunk through the scalar cache).
// SCH: the block schedule of the transforming forms with one sub-tile of loads in flight (chain_v4_sched below picks it):
//   0  the sub-tile loop: a step's place in its block is a run-time fact (the register shift, the (j & 3) test), the transform's
//      middle-stage twiddles are global loads behind the stream request;
//   1  a loop over whole blocks of four steps whose place S is a compile-time fact: the FIR's results go straight to a[4 S ...], and the
//      loop issues no global load but the stream (middle-stage twiddles from the LDS table PF2 uses, tw[0] resident);
//   2  1, and the transform of block b runs UNDER the FIR of block b + 1's first sub-tile, piece by piece between that window's read
//      chunks (fft1kn_wave_piece through the FIR's per-chunk hook), its exchanges in halves behind the image -- which stays intact, so
//      the halo is never held in registers across a transform.  A run's last block has no next FIR and transforms as in 1.
// One body for the single-message kernels, the list kernel and their any-taps twins; `wave` is the wavefront's index within its
// message (the workgroup index of a single-message launch).
template <int K, int D, bool FUSED, int WPS, int CH, bool FIR_ONLY, bool TWP, bool IN_U8, bool PF2, bool RES, int SCH>
__device__ __forceinline__ void chain_v4_body(const float2 *__restrict__ x, const float *__restrict__ taps,
                                              const float2 *__restrict__ tw, float2 *__restrict__ out,
                                              long nblocks, long blocks_per_wave, long wave, unsigned long long *dbg, long dbg_cap)
{
    // diagnostic only (dbg != nullptr): shader-clock and 100 MHz real-time stamps around the wave's life,
    // written to a buffer of their own; run times of such launches are never quoted
    unsigned long long t0c = 0, t0r = 0;
    if (dbg) { t0c = __builtin_amdgcn_s_memtime(); t0r = __builtin_amdgcn_s_memrealtime(); }
    constexpr int R = 4;
    using G = FirGeomV<K, D, R>;
    constexpr int SUB_OUT = 64 * R;                   // 256 outputs per sub-tile
    constexpr int SUB_NEW = SUB_OUT * D;              // 1280 new input samples per sub-tile
    constexpr int HALO = G::tile_in(SUB_OUT) - SUB_NEW; // 122 samples shared with the previous sub-tile
    static_assert(HALO % 2 == 0 && SUB_NEW % 128 == 0 && 4 * SUB_OUT == 1024, "geometry");
    constexpr int HALO_V = HALO / 2;                  // 61 float4
    constexpr int NLD = SUB_NEW / 2 / 64;             // 10 float4 per lane
    static_assert(HALO_V <= 64, "the halo moves with one instruction per lane");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v4f_t *xs4 = reinterpret_cast<v4f_t *>(smem);
    float2 *ex = reinterpret_cast<float2 *>(smem);

    const int lane = threadIdx.x;
    const long b0 = wave * blocks_per_wave;
    if (b0 >= nblocks) return;
    const long b1 = (b0 + blocks_per_wave < nblocks) ? b0 + blocks_per_wave : nblocks;
    const long nsub = 4 * (b1 - b0);                  // sub-tiles of this wave, consecutive in the stream
    // the ceil(K/2) distinct taps, once per wave (the any-taps kernels carry no resident state)
    typename std::conditional<RES, FirTapsResident<K>, FirNoResidentTaps>::type rtaps;
    if constexpr (RES) fir_taps_resident_load(rtaps, taps);
    // index of the first NEW pair of samples of sub-tile j (the halo precedes it): a pair is one float4, or one u32 of I/Q bytes
    using pair_t = typename std::conditional<IN_U8, unsigned, v4f_t>::type;
    [[maybe_unused]] const pair_t *src0 = (IN_U8 ? reinterpret_cast<const pair_t *>(reinterpret_cast<const unsigned *>(x) + b0 * 512 * (long)D)
                                : reinterpret_cast<const pair_t *>(x + b0 * 1024 * (long)D)) + lane;
    auto samples = [](pair_t w) -> v4f_t {
        if constexpr (IN_U8) return v4f_t{i2f(w & 255u), i2f((w >> 8) & 255u), i2f((w >> 16) & 255u), i2f(w >> 24)};
        else return w;
    };

    constexpr bool HOIST = (REDIO_EXP_SEAM & 1) != 0, BUF = PF2 || (REDIO_EXP_SEAM & 2) != 0, EARLY = (REDIO_EXP_SEAM & 4) != 0,
                   PRO = (REDIO_EXP_SEAM & 8) != 0;
    // image slot (16-byte units) of sample pair p.  Two facts about it make a wave's slots few:
    //   the halo's source is its destination HALO_DELTA slots on (SUB_NEW / 2 pairs are a whole number of lane strides), and
    //   park slots i and i + PER are PARK_STEP apart (so are 64 PER pairs): NLD stores share PER address registers, the rest is immediates.
    auto slot = [](int p) { return G::lds_index(2 * p) / 2; };
    constexpr int HSTR = G::LSTR / 2; // pairs per lane stride
    static_assert((SUB_NEW / 2) % HSTR == 0, "a sub-tile is a whole number of lane strides");
    constexpr int HALO_DELTA = G::lds_index(SUB_NEW) / 2;
    constexpr int PER0 = G::PADN == 0 ? 1 : HSTR / chain_gcd(64, HSTR), PER = PER0 < NLD ? PER0 : NLD;
    constexpr int PARK_STEP = G::lds_index(2 * 64 * PER) / 2;
    static_assert(PER == NLD || (64 * PER) % HSTR == 0, "park slots repeat with period PER");
    // HOIST: lane-constant for the life of the wave.  The halo move is branch-free (EARLY): the lanes behind the halo move a pair of
    // NEW samples onto itself, harmless because the park that follows writes that slot again (one wave's LDS operations execute in
    // issue order, fft_wave.h wave_lds_fence) -- no slot outside the image is needed.
    auto halo_slots = [&](int lf, int &src, int &dst) {
        dst = slot(lf);
        if constexpr (EARLY) src = dst + (lf < HALO_V ? HALO_DELTA : 0);
        else src = slot(SUB_NEW / 2 + lf);
    };
    [[maybe_unused]] int park4[PER], hsrc4 = 0, hdst4 = 0;
    if constexpr (HOIST) {
        static_for4<PER>([&](auto I) { park4[I.value] = slot(HALO_V + lane + 64 * I.value); });
        halo_slots(lane, hsrc4, hdst4);
    }

    pair_t pre[NLD], pre2[PF2 ? NLD : 1];
    // BUF: the stream is read, and the output written, through buffer descriptors of the wave's own run -- input [head of sub-tile 0,
    // end of sub-tile nsub - 1), output its b1 - b0 blocks.  An access is descriptor base + scalar offset + (lane offset + immediate):
    // the wave-uniform part lives in scalar registers and the lane part is ONE constant register, so the loop has no vector address
    // arithmetic.  The scalar offset is NOT range-checked, so nothing here relies on the check: every request lies inside the run.
    // PF2 keeps the sub-tile's offset in the lane part, which IS checked: a request for a sub-tile behind the run's last one (the last two
    // steps of a run ask for them) lies past num_records and returns zeros WITHOUT a memory access, so every PF2 step requests
    // unconditionally and the number of loads in flight at every wait is a compile-time fact (a request under a condition makes the
    // compiler wait for ALL loads at the next use, i.e. also for the request it issued a sub-tile ago -- the whole point of the second set)
    constexpr unsigned PB = sizeof(pair_t);                        // bytes of a pair in the stream
    constexpr int NT_LD = (REDIO_EXP_CHAIN_NT & 1) ? 2 : 0, NT_ST = (REDIO_EXP_CHAIN_NT & 2) ? 2 : 0; // the buffer forms' cache-policy operand: nt
    typedef unsigned v4u_t __attribute__((ext_vector_type(4)));
    typedef unsigned v2u_t __attribute__((ext_vector_type(2)));
    [[maybe_unused]] __amdgpu_buffer_rsrc_t ri, ro;
    if constexpr (BUF) {
        static_assert(!PF2 || !IN_U8, "PF2: cf32 input");
        const char *xb = reinterpret_cast<const char *>(x) + b0 * (512 * (long)D) * PB;
        ri = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(xb), 0, (int)((HALO_V + nsub * (SUB_NEW / 2)) * PB), 0x00020000);
        ro = __builtin_amdgcn_make_buffer_rsrc(out + b0 * 1024, 0, (int)((b1 - b0) * 8192), 0x00020000);
    }
    [[maybe_unused]] auto buf_load = [&](unsigned vo, unsigned so, auto policy) -> pair_t {
        if constexpr (IN_U8) return __builtin_amdgcn_raw_buffer_load_b32(ri, vo, so, decltype(policy)::value);
        else return __builtin_bit_cast(v4f_t, __builtin_amdgcn_raw_buffer_load_b128(ri, vo, so, decltype(policy)::value));
    };
    auto fetch_to = [&](pair_t(&dst)[NLD], long j) { // new samples of sub-tile j: [HALO + j*SUB_NEW, HALO + (j+1)*SUB_NEW)
        if constexpr (BUF) {
            const unsigned sub = (unsigned)((HALO_V + j * (SUB_NEW / 2)) * PB); // wave-uniform
            const unsigned vo = PB * (unsigned)lane + (PF2 ? sub : 0u), so = PF2 ? 0u : sub;
            static_for4<NLD>([&](auto I) {
                constexpr unsigned off = 64u * PB * I.value, imm = off % 4096u; // load k: an immediate below 4096 and a scalar multiple of it
                dst[I.value] = buf_load(vo + imm, so + (off - imm), std::integral_constant<int, NT_LD>{});
                // in ascending address order, as the parent's loads went out: left alone the scheduler groups them by scalar offset, two
                // loads that share a 128-byte line are then no longer neighbours, and FETCH_SIZE rises by 0.6 % (r12_chain_seam.txt)
                if constexpr (!PF2) __builtin_amdgcn_sched_barrier(0);
            });
        } else {
            const pair_t *src = src0 + HALO_V + j * (SUB_NEW / 2);
            // the stream is read once: non-temporal loads (round 3: read streams run 5-9 % faster with them on this part,
            // profiles/r03_stream_probe3.txt; -DREDIO_EXP_CHAIN_NT=0 builds the default-policy form for comparison)
#if REDIO_EXP_CHAIN_NT & 1
            static_for4<NLD>([&](auto I) { dst[I.value] = __builtin_nontemporal_load(src + 64 * I.value); });
#else
            static_for4<NLD>([&](auto I) { dst[I.value] = src[64 * I.value]; });
#endif
        }
    };
    auto park_from = [&](pair_t(&from)[NLD]) {
#if REDIO_EXP_ABLATE == 3 // timing-only experiment (tools/chain_variants.sh; results WRONG): the loads stay, the ten ds_write_b128 that
                          // park them in the image do not -- an upper bound on what staging by LDS-DMA instead of registers could buy
#pragma unroll
        for (int i = 0; i < NLD; ++i) { pair_t keep = from[i]; asm volatile("" : : "v"(keep)); }
#else
        static_for4<NLD>([&](auto I) {
            constexpr int i = I.value;
            if constexpr (HOIST) xs4[park4[i % PER] + (i / PER) * PARK_STEP] = samples(from[i]);
            else xs4[G::lds_index(HALO + 2 * (lane + 64 * i)) / 2] = samples(from[i]);
        });
#endif
    };
    // a block's spectrum, a[k1 + 4 k0] = X[ln + 64 k1 + 256 k0] (fft1kn_store_spectrum's order); blk: the block's place in the run
    [[maybe_unused]] auto store_block = [&](const float2(&a)[16], long blk, int ln) {
        if constexpr (BUF) {
            const unsigned so = (unsigned)(blk * 8192); // wave-uniform
            static_for4<16>([&](auto I) {
                constexpr unsigned k0 = I.value / 4, k1 = I.value % 4;
                const float2 v = a[k1 + 4 * k0];
                __builtin_amdgcn_raw_buffer_store_b64(v2u_t{__builtin_bit_cast(unsigned, v.x), __builtin_bit_cast(unsigned, v.y)}, ro,
                                                      8u * (unsigned)ln + (512u * k1 + 2048u * (k0 & 1)), so + 4096u * (k0 >> 1), NT_ST);
            });
        } else fft1kn_store_spectrum(a, out + (b0 + blk) * 1024, ln);
    };

    // PF2, SCH 1, 2: the 60 twiddles of the transform's middle stages (Fft1knTw12: 15 per lane, 4 distinct sets by lane >> 4) sit in LDS behind the
    // image for the life of the wave, so the transform issues NO global load: its twiddle loads would queue behind the sub-tile request
    // (loads return in order) and make the transform wait for it
    static_assert(SCH == 0 || (!PF2 && !FIR_ONLY && TWP && WPS == 2), "the block schedules: the transforming product forms");
    constexpr int EXH_OFF = G::lds_elems(SUB_OUT) > FFT1KN_LDS ? G::lds_elems(SUB_OUT) : FFT1KN_LDS; // SCH 2: the half exchanges, behind image and one-piece exchange
    constexpr int T12_OFF = EXH_OFF + (SCH == 2 ? FFT1KN_HALF_LDS : 0);
    constexpr bool TABLE = (PF2 || SCH != 0) && !FIR_ONLY;
    // (64 entries: the PRO prologue stores with all lanes, the last four land in a pad behind the table; PF2's request has room for them too)
    static_assert(!TABLE || (T12_OFF + 64) * sizeof(float2) <= 160 * 1024 / 8 - 480, "within the request of chain_v4_lds at two waves per SIMD");
    auto table_index = [](int l) { // of the table's entry l in tw
        const int k4 = l / 15, i = l % 15;
        return i < 3 ? 64 * k4 * (i + 1) : 16 * (k4 + 4 * ((i - 3) / 3)) * ((i - 3) % 3 + 1);
    };
    // the 15 lane-dependent twiddles of the last two stages stay in registers for the life of the wave
    Fft1knTw34 t34;
    // SCH 1, 2: tw[0] (the first stage's unit twiddle) in two registers and the middle-stage twiddles from the LDS table, so that a block's
    // transform issues no global load
    [[maybe_unused]] float2 one = make_float2(0.f, 0.f);
    // prologue: the head (the only halo this wave ever fetches), the first sub-tile, the twiddles
    if constexpr (PRO) {
        // Every request before the first wait, the stream's first: one memory latency, not one each for head, table and sub-tile.
        // All 64 lanes fetch and store a head pair: the lanes behind the halo hold the first NEW pairs, which the park writes again.
        pair_t head;
        if constexpr (BUF) head = buf_load(PB * (unsigned)lane, 0u, std::integral_constant<int, 0>{});
        else head = src0[0];
        fetch_to(pre, 0);
        [[maybe_unused]] float2 twv = make_float2(0.f, 0.f);
        if constexpr (TABLE) twv = tw[table_index(lane < 60 ? lane : 0)];
        if (!FIR_ONLY && TWP) fft1kn_load_tw34(t34, lane, tw);
        if constexpr (SCH != 0) one = tw[0];
        xs4[slot(lane)] = samples(head);
        if constexpr (TABLE) ex[T12_OFF + lane] = twv; // all lanes: under a lane mask the compiler moves the load into the masked block, behind a wait of its own
        park_from(pre);
        wave_lds_fence();
    } else {
        if (lane < HALO_V) {
            if constexpr (BUF) xs4[slot(lane)] = samples(buf_load(PB * (unsigned)lane, 0u, std::integral_constant<int, 0>{}));
            else xs4[slot(lane)] = samples(src0[0]);
        }
        if constexpr (TABLE)
            if (lane < 60) ex[T12_OFF + lane] = tw[table_index(lane)];
        fetch_to(pre, 0);
        park_from(pre);
        wave_lds_fence();
        if (!FIR_ONLY && TWP) fft1kn_load_tw34(t34, lane, tw);
        if constexpr (SCH != 0) one = tw[0];
    }
    if constexpr (SCH != 0) asm volatile("" : "+v"(one.x), "+v"(one.y));

    // the block in the transform's operand layout; SCH 1 writes all of it before its first transform, the sub-tile loops shift it in
    float2 a[16];
    if constexpr (!(PRO && SCH == 1)) {
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = make_float2(0.f, 0.f);
    }
    // one sub-tile: request sub-tile j + AHEAD into `req`, FIR of the image, transform when a block is complete,
    // then park `parked` (= sub-tile j + 1, requested AHEAD - 1 sub-tiles ago; for AHEAD == 1 it is `req` itself) into the image.
    // S: the sub-tile's place in its block when that is a compile-time fact (PF2: the loop below is unrolled by a whole block, the
    // transform sits in step 3 unconditionally, and so do the request, the halo move and the park), -1 when it is not.
    // The seam of a step: the FIR of the image and the move of the image's last HALO samples, the next image's first.
    //   EARLY: the halo is read under the FIR's last chunk (fir_core.h's per-chunk hook), so it has long arrived when the window's last
    //          multiply-add has; its write goes out behind the last window read with nothing to wait for, all 64 lanes (halo_slots).
    //   else:  read behind the window under the lane mask, waited for, written under the mask (the parent's form).
    // !HOIST: the slots are recomputed every step from an opaque copy of the lane (the parent's form: out of the loop's live set).
    constexpr int NCH = fir_num_chunks<K, D, R, CH>();
    struct Seam { int lf, hs, hd; v4f_t halo; };
    auto fir = [&](Seam &s, float2(&acc)[R], auto &&hook) {
        s.lf = lane, s.hs = hsrc4, s.hd = hdst4, s.halo = v4f_t{0.f, 0.f, 0.f, 0.f};
        if constexpr (!HOIST) {
            asm volatile("" : "+v"(s.lf));
            if constexpr (EARLY) halo_slots(s.lf, s.hs, s.hd);
        }
        auto hk = [&](auto C) {
            if constexpr (EARLY && decltype(C)::value == NCH - 1) s.halo = xs4[s.hs];
            hook(C);
        };
        if constexpr (RES) fir_lane_v_res<K, D, R, FUSED, CH>(xs4, s.lf, rtaps, acc, hk);
        else fir_lane_v<K, D, R, FUSED, CH>(xs4, s.lf, taps, acc, hk);
    };
    auto halo_read = [&](Seam &s, bool more) { // behind the fence that ends the window reads
        if constexpr (!EARLY) {
            if constexpr (!HOIST) halo_slots(s.lf, s.hs, s.hd);
            if (more && s.lf < HALO_V) s.halo = xs4[s.hs];
        }
    };
    auto halo_write = [&](const Seam &s) {
        if constexpr (EARLY) xs4[s.hd] = s.halo;
        else if (s.lf < HALO_V) xs4[HOIST ? s.hd : slot(s.lf)] = s.halo;
    };
    auto transform_lane = [&]() { // !HOIST: opaque per transform, so that the exchanges' address arithmetic stays out of the live set
        int ln = lane;
        if constexpr (!HOIST) asm volatile("" : "+v"(ln));
        return ln;
    };
    // one sub-tile: request sub-tile j + AHEAD into `req`, FIR of the image, transform when a block is complete,
    // then park `parked` (= sub-tile j + 1, requested AHEAD - 1 sub-tiles ago; for AHEAD == 1 it is `req` itself) into the image.
    // S: the sub-tile's place in its block when that is a compile-time fact (PF2: the loop below is unrolled by a whole block, the
    // transform sits in step 3 unconditionally, and so do the request, the halo move and the park), -1 when it is not.
    auto step = [&](long j, auto ahead, auto place, pair_t(&req)[NLD], pair_t(&parked)[NLD]) {
        constexpr int AHEAD = decltype(ahead)::value, S = decltype(place)::value;
        const bool more = S >= 0 || j + 1 < nsub;
        if (S >= 0 || j + AHEAD < nsub) fetch_to(req, j + AHEAD);
        float2 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);
        Seam seam;
        fir(seam, acc, FirNoHook{});
        if (FIR_ONLY) { // 32 contiguous bytes per lane, 2 KiB per wave
            const v4f_t y0 = v4f_t{acc[0].x, acc[0].y, acc[1].x, acc[1].y}, y1 = v4f_t{acc[2].x, acc[2].y, acc[3].x, acc[3].y};
            if constexpr (BUF) {
                const unsigned so = (unsigned)(j * (SUB_OUT * 8)); // wave-uniform
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, y0), ro, 32u * (unsigned)lane, so, 0);
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u_t, y1), ro, 32u * (unsigned)lane + 16u, so, 0);
            } else {
                v4f_t *y4 = reinterpret_cast<v4f_t *>(out + (b0 * 4 + j) * SUB_OUT) + 2 * lane;
                y4[0] = y0;
                y4[1] = y1;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) a[i] = a[i + 4];
#pragma unroll
            for (int r = 0; r < R; ++r) a[12 + r] = acc[r];
        }
        wave_lds_fence(); // window reads done
        halo_read(seam, more);
        if (!FIR_ONLY && (S == 3 || (S < 0 && (j & 3) == 3))) { // a block is complete in registers: transform it, the image is scratch meanwhile
            wave_lds_fence();
            const int ln = transform_lane();
            Fft1knTw12 t12;
            if constexpr (PF2) {
                const float2 *T = ex + T12_OFF + 15 * (ln >> 4);
#pragma unroll
                for (int i = 0; i < 3; ++i) t12.a[i] = T[i];
#pragma unroll
                for (int i = 0; i < 12; ++i) t12.b[i] = T[3 + i];
            } else fft1kn_load_tw12(t12, ln, tw);
            if (!TWP) fft1kn_load_tw34(t34, ln, tw);
            fft1kn_wave_regs<false>(a, ex, tw, t12, t34, ln);
            store_block(a, j >> 2, ln);
            wave_lds_fence();
        }
        if (more) {
            halo_write(seam);
            park_from(parked);
        }
        wave_lds_fence();
    };
    [[maybe_unused]] auto t12_lds = [&](Fft1knTw12 &t12, int ln) {
        const float2 *T = ex + T12_OFF + 15 * (ln >> 4);
#pragma unroll
        for (int i = 0; i < 3; ++i) t12.a[i] = T[i];
#pragma unroll
        for (int i = 0; i < 12; ++i) t12.b[i] = T[3 + i];
    };
    // SCH 1, 2: one sub-tile at place S of its block.  more: another sub-tile follows in this run (S < 3: always); xform: the block
    // completed by this step (S == 3) is transformed here, the image its scratch and the halo held meanwhile; hook: fir_core.h
    [[maybe_unused]] auto sstep = [&](long j, auto place, bool more_, bool xform_, auto &&hook) {
        constexpr int S = decltype(place)::value;
        const bool more = S < 3 || more_, xform = S == 3 && xform_;
        if (more) fetch_to(pre, j + 1);
        float2 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = make_float2(0.f, 0.f);
        Seam seam;
        fir(seam, acc, hook);
#pragma unroll
        for (int r = 0; r < R; ++r) a[4 * S + r] = acc[r];
        wave_lds_fence(); // window reads done
        halo_read(seam, more);
        if (xform) {
            wave_lds_fence();
            const int ln = transform_lane();
            Fft1knTw12 t12;
            t12_lds(t12, ln);
            const float2 one1[1] = {one};
            fft1kn_wave_regs<false>(a, ex, one1, t12, t34, ln);
            store_block(a, j >> 2, ln);
            wave_lds_fence();
        }
        if (more) {
            halo_write(seam);
            park_from(pre);
        }
        wave_lds_fence();
    };
    using S0 = std::integral_constant<int, 0>;
    using S1 = std::integral_constant<int, 1>;
    using S2 = std::integral_constant<int, 2>;
    using S3 = std::integral_constant<int, 3>;
    if constexpr (SCH == 1) {
        const long nb = b1 - b0;
#pragma unroll 1
        for (long blk = 0; blk < nb; ++blk) {
            sstep(4 * blk, S0{}, true, false, FirNoHook{});
            sstep(4 * blk + 1, S1{}, true, false, FirNoHook{});
            sstep(4 * blk + 2, S2{}, true, false, FirNoHook{});
            sstep(4 * blk + 3, S3{}, blk + 1 < nb, true, FirNoHook{});
        }
    } else if constexpr (SCH == 2) {
        const long nb = b1 - b0;
        sstep(0, S0{}, true, false, FirNoHook{});
#pragma unroll 1
        for (long blk = 0;; ++blk) {
            sstep(4 * blk + 1, S1{}, true, false, FirNoHook{});
            sstep(4 * blk + 2, S2{}, true, false, FirNoHook{});
            const bool more = blk + 1 < nb;
            sstep(4 * blk + 3, S3{}, more, !more, FirNoHook{}); // the run's last block: transformed there
            if (!more) break;
            // block blk under the first FIR of block blk + 1
            float2 ap[16], u[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) ap[i] = a[i];
            int ln = lane;
            asm volatile("" : "+v"(ln));
            Fft1knTw12 t12;
            float2 *dst = out + (b0 + blk) * 1024;
            auto piece = [&](auto C) {
                fft1kn_wave_piece<decltype(C)::value, false>(ap, u, ex + EXH_OFF, one, ex + T12_OFF + 15 * (ln >> 4), t12, t34, dst, ln);
            };
            sstep(4 * blk + 4, S0{}, true, false, piece);
            if constexpr (NCH < FFT1KN_PIECES) // a window of fewer chunks than the transform has pieces: the rest behind it
                static_for4<FFT1KN_PIECES - NCH>([&](auto I) { piece(std::integral_constant<int, NCH + I.value>{}); });
        }
    } else if constexpr (PF2) {
        fetch_to(pre, 1);
        using two = std::integral_constant<int, 2>;
#pragma unroll 1
        for (long j = 0; j < nsub; j += 4) { // one block per iteration
            step(j, two{}, std::integral_constant<int, 0>{}, pre2, pre);
            step(j + 1, two{}, std::integral_constant<int, 1>{}, pre, pre2);
            step(j + 2, two{}, std::integral_constant<int, 2>{}, pre2, pre);
            step(j + 3, two{}, std::integral_constant<int, 3>{}, pre, pre2);
        }
    } else {
#pragma unroll 1
        for (long j = 0; j < nsub; ++j) step(j, std::integral_constant<int, 1>{}, std::integral_constant<int, -1>{}, pre, pre);
    }
    if (dbg && lane == 0 && (long)blockIdx.x < dbg_cap) { // the caller's buffer holds dbg_cap records: later waves leave no stamp
        dbg[4 * blockIdx.x] = __builtin_amdgcn_s_memtime() - t0c;
        dbg[4 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - t0r;
        dbg[4 * blockIdx.x + 2] = t0r; // absolute start (100 MHz ticks)
        unsigned xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned hwid = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
        dbg[4 * blockIdx.x + 3] = ((unsigned long long)xcc << 32) | hwid;
    }
}

// The block schedule (chain_v4_body, SCH) of a kernel's template parameters: one rule for the single-message kernels, the list
// kernels and the any-taps twins.  The transforming product forms run schedule 1 (round 8: - 1.1 % on the headline kernel, every run
// beyond the parent's range); schedule 2 measured no better than 1 (profiles/r08_chain_block_schedule.txt) and is built only as
// chain_v4_sched2_kernel of the measurement build.
template <int WPS, bool FIR_ONLY, bool TWP, bool PF2, bool RES>
constexpr int chain_v4_sched()
{
    return (WPS == 2 && !FIR_ONLY && TWP && !PF2) ? 1 : 0;
}

// PRECONDITION: bit-palindromic taps (chain_v4_body, RES).  The template parameters, and so the name a profiler prints, are those of
// the kernel before the resident-taps form.
template <int K, int D, bool FUSED, int WPS, int CH, bool FIR_ONLY = false, bool TWP = false, bool IN_U8 = false, bool PF2 = false>
__global__ __launch_bounds__(64, WPS) void chain_v4_kernel(const float2 *__restrict__ x, const float *__restrict__ taps,
                                                           const float2 *__restrict__ tw, float2 *__restrict__ out,
                                                           long nblocks, long blocks_per_wave, unsigned long long *dbg, long dbg_cap)
{
    chain_v4_body<K, D, FUSED, WPS, CH, FIR_ONLY, TWP, IN_U8, PF2, true, chain_v4_sched<WPS, FIR_ONLY, TWP, PF2, true>()>(x, taps, tw, out, nblocks, blocks_per_wave, (long)blockIdx.x, dbg, dbg_cap);
}
// any taps: the plans whose taps are not bit-palindromic
template <int K, int D, bool FUSED, int WPS, int CH, bool FIR_ONLY = false, bool TWP = false, bool IN_U8 = false, bool PF2 = false>
__global__ __launch_bounds__(64, WPS) void chain_v4_anytaps_kernel(const float2 *__restrict__ x, const float *__restrict__ taps,
                                                                   const float2 *__restrict__ tw, float2 *__restrict__ out,
                                                                   long nblocks, long blocks_per_wave, unsigned long long *dbg, long dbg_cap)
{
    chain_v4_body<K, D, FUSED, WPS, CH, FIR_ONLY, TWP, IN_U8, PF2, false, chain_v4_sched<WPS, FIR_ONLY, TWP, PF2, false>()>(x, taps, tw, out, nblocks, blocks_per_wave, (long)blockIdx.x, dbg, dbg_cap);
}

#ifdef REDIO_MEASURE
// schedule 2 (the transform of block b under the first FIR of block b + 1) on the headline shape, resident taps: A/B against the product
// form in one process, tools/chain_sched_ab.py
template <int K, int D, bool FUSED>
__global__ __launch_bounds__(64, 2) void chain_v4_sched2_kernel(const float2 *__restrict__ x, const float *__restrict__ taps,
                                                                const float2 *__restrict__ tw, float2 *__restrict__ out,
                                                                long nblocks, long blocks_per_wave, unsigned long long *dbg, long dbg_cap)
{
    chain_v4_body<K, D, FUSED, 2, 8, false, true, false, false, true, 2>(x, taps, tw, out, nblocks, blocks_per_wave, (long)blockIdx.x, dbg, dbg_cap);
}
#endif

// A list of independent cf32 messages in ONE launch (redio_chain_enqueue_list): message i owns the waves [wave0[i], wave0[i + 1]).
// The list travels by value in the kernel arguments: no descriptor buffer, nothing to upload or recycle, and a captured launch carries
// its own copy.
struct ChainList {
    const float2 *x[REDIO_LIST_MAX];
    float2 *out[REDIO_LIST_MAX];
    long nblocks[REDIO_LIST_MAX];
    unsigned wave0[REDIO_LIST_MAX + 1]; // wave-start prefix: wave0[count] = the launch's waves
    int count;
};

// A wave runs exactly what chain_v4_kernel<K, D, FUSED, 2, 8, false, true> runs for (x_i, out_i, nblocks_i, blocks_per_wave): the same
// body, so the bits are those of one launch per message; a wave never spans two messages.
template <int K, int D, bool FUSED, bool RES>
__device__ __forceinline__ void chain_v4_list_body(const ChainList &list, const float *__restrict__ taps, const float2 *__restrict__ tw,
                                                   long blocks_per_wave)
{
    // which message: a scan of the wave-start prefix in scalar registers (the workgroup index and the list are wave-uniform)
    const unsigned w = blockIdx.x;
    int m = 0;
    for (int i = 1; i < list.count; ++i) m = w >= list.wave0[i] ? i : m;
    m = __builtin_amdgcn_readfirstlane(m);
    // wave index within the message: b0 < nblocks, the host gives message i ceil(nblocks_i / bpw) waves
    chain_v4_body<K, D, FUSED, 2, 8, false, true, false, false, RES, chain_v4_sched<2, false, true, false, RES>()>(list.x[m], taps, tw, list.out[m], list.nblocks[m], blocks_per_wave,
                                                                     (long)(w - list.wave0[m]), nullptr, 0);
}

// PRECONDITION: bit-palindromic taps (chain_v4_body, RES)
template <int K, int D, bool FUSED>
__global__ __launch_bounds__(64, 2) void chain_v4_list_kernel(const ChainList list, const float *__restrict__ taps,
                                                              const float2 *__restrict__ tw, long blocks_per_wave)
{
    chain_v4_list_body<K, D, FUSED, true>(list, taps, tw, blocks_per_wave);
}
// any taps
template <int K, int D, bool FUSED>
__global__ __launch_bounds__(64, 2) void chain_v4_anytaps_list_kernel(const ChainList list, const float *__restrict__ taps,
                                                                      const float2 *__restrict__ tw, long blocks_per_wave)
{
    chain_v4_list_body<K, D, FUSED, false>(list, taps, tw, blocks_per_wave);
}

// blocks per wavefront of a launch over nblocks blocks at WPS wavefronts per SIMD (the chain: 2; the FIR alone: 3)
long chain_v4_blocks_per_wave(long nblocks, int WPS)
{
    // Short runs in dispatch order, not one long run per residency slot: the wavefronts resident at any moment then read one
    // compact window of the stream (2048 x 4 blocks = 335 MB apart at most, instead of 2048 places spread over all of it).
    // Measured with non-temporal accesses 0.533 -> 0.517 ms per 2^28 samples (profiles/r03_chain_variants.txt); a run
    // re-fetches its 122-sample head: 0.6 % more reads at four blocks per run.
    long waves = 4L * WPS * num_cus();
    if (waves > nblocks) waves = nblocks;
    if (waves < 1) waves = 1;
    // ... and at least about six sets of wavefronts per launch: with fewer the last, partly filled set is most of a run's length of idle
    // slots (2^26 samples, 127 taps / 5 alone: 0.153-0.159 ms at four blocks per run, 0.131-0.139 at one; 63 taps / 5: 0.137 -> 0.117)
    long bpw = nblocks / (6 * waves);
    if (bpw < 1) bpw = 1;
    if (bpw > 4) bpw = 4;
    if (const char *e = measure_env("REDIO_CHAIN_BPW")) { const long v = atol(e); if (v >= 1) bpw = v; } // -DREDIO_MEASURE builds only: blocks per wavefront
    return bpw;
}

// dynamic LDS of one wavefront of the kernels above
template <int K, int D, int WPS, bool PF2 = false>
static constexpr size_t chain_v4_lds()
{
    static_assert(WPS == 2 || WPS == 3, "two wavefronts per SIMD (the chain: its transform needs 197 registers) or three (the FIR alone: 94-145)");
    using G = FirGeomV<K, D, 4>;
    constexpr int ELEMS = (G::lds_elems(256) > FFT1KN_LDS ? G::lds_elems(256) : FFT1KN_LDS) + (PF2 ? 64 : 0); // PF2: the middle stages' twiddles behind the image
    constexpr size_t LDS_NEED = (size_t)ELEMS * sizeof(float2);
    static_assert(4 * WPS * LDS_NEED <= 160 * 1024, "4*WPS waves per CU");
    // The grid is exactly one wave per residency slot.  Ask for 1/(4*WPS) of the CU's LDS (minus a
    // margin for allocation granularity) so that a CU can NOT take more than 4*WPS waves: without this
    // the dispatcher packs up to 12-13 of these small workgroups on some CUs and leaves others
    // half empty, and the launch ends when the most crowded CU does (measured: wave lifetimes 320-570 us).
    constexpr size_t LDS = (160 * 1024 / (4 * WPS)) - 480 > LDS_NEED ? (160 * 1024 / (4 * WPS)) - 480 : LDS_NEED;
    static_assert((4 * WPS + 1) * LDS > 160 * 1024, "one more wave must not fit");
    return LDS;
}

// pal: the plan's taps are bit-palindromic (decided once at plan creation): the resident-taps kernel, whose precondition that is; else its any-taps twin
template <int K, int D, int WPS, int CH, bool FIR_ONLY = false, bool TWP = false, bool IN_U8 = false, bool PF2 = false>
static hipError_t launch_v4_t(const float2 *x, const float *taps, bool pal, const float2 *tw, float2 *out, long nblocks, bool fused,
                              hipStream_t s, unsigned long long *dbg, long dbg_cap = 0)
{
    constexpr size_t LDS = chain_v4_lds<K, D, WPS, PF2>();
    const long bpw = chain_v4_blocks_per_wave(nblocks, WPS);
    const long grid = (nblocks + bpw - 1) / bpw;
    if (pal) {
        if (fused) hipLaunchKernelGGL((chain_v4_kernel<K, D, true, WPS, CH, FIR_ONLY, TWP, IN_U8, PF2>), dim3((unsigned)grid), dim3(64), LDS, s, x, taps, tw, out, nblocks, bpw, dbg, dbg_cap);
        else hipLaunchKernelGGL((chain_v4_kernel<K, D, false, WPS, CH, FIR_ONLY, TWP, IN_U8, PF2>), dim3((unsigned)grid), dim3(64), LDS, s, x, taps, tw, out, nblocks, bpw, dbg, dbg_cap);
    } else {
        if (fused) hipLaunchKernelGGL((chain_v4_anytaps_kernel<K, D, true, WPS, CH, FIR_ONLY, TWP, IN_U8, PF2>), dim3((unsigned)grid), dim3(64), LDS, s, x, taps, tw, out, nblocks, bpw, dbg, dbg_cap);
        else hipLaunchKernelGGL((chain_v4_anytaps_kernel<K, D, false, WPS, CH, FIR_ONLY, TWP, IN_U8, PF2>), dim3((unsigned)grid), dim3(64), LDS, s, x, taps, tw, out, nblocks, bpw, dbg, dbg_cap);
    }
    return hipGetLastError();
}

hipError_t launch_chain_v4(const float2 *x, const float *taps, bool pal, const float2 *tw, float2 *out, long nblocks, bool fused,
                           hipStream_t s, unsigned long long *dbg, long dbg_cap)
{
    // (three wavefronts per SIMD were measured again in round 3 with the new access policy: the transform's registers spill at
    // 168 per lane, 0.56-0.60 against 0.517 ms)
#ifdef REDIO_MEASURE // three wavefronts per SIMD without the resident last-stage twiddles (168 registers, 80 bytes of scratch): measured in round 4, see DESIGN.md 5.1
    if (measure_env("REDIO_CHAIN_WPS3")) return launch_v4_t<127, 5, 3, 8, false, false>(x, taps, pal, tw, out, nblocks, fused, s, dbg, dbg_cap);
    // two sub-tiles of loads in flight (round 6): A/B against the product form in one process, tools/chain_pf2_ab.py
    if (measure_env("REDIO_CHAIN_PF2")) return launch_v4_t<127, 5, 2, 8, false, true, false, true>(x, taps, pal, tw, out, nblocks, fused, s, dbg, dbg_cap);
    // the transform under the next FIR (round 8): the product form's geometry and LDS request
    if (pal && measure_env("REDIO_CHAIN_SCHED2")) {
        const long bpw = chain_v4_blocks_per_wave(nblocks, 2);
        const dim3 grid((unsigned)((nblocks + bpw - 1) / bpw));
        if (fused) hipLaunchKernelGGL((chain_v4_sched2_kernel<127, 5, true>), grid, dim3(64), (chain_v4_lds<127, 5, 2>()), s, x, taps, tw, out, nblocks, bpw, dbg, dbg_cap);
        else hipLaunchKernelGGL((chain_v4_sched2_kernel<127, 5, false>), grid, dim3(64), (chain_v4_lds<127, 5, 2>()), s, x, taps, tw, out, nblocks, bpw, dbg, dbg_cap);
        return hipGetLastError();
    }
#endif
    return launch_v4_t<127, 5, 2, 8, false, true>(x, taps, pal, tw, out, nblocks, fused, s, dbg, dbg_cap); // last-stage twiddles resident
}

// u8 I/Q bytes in (4-byte aligned), spectra out: data_to_samples -> 127-tap FIR / 5 -> 1024-point FFT in one kernel
// pal, here and in every launcher of this file: the plan's taps are bit-palindromic (the precondition of chain_v4_kernel); false selects
// chain_v4_anytaps_kernel
hipError_t launch_chain_v4_u8(const void *bytes, const float *taps, bool pal, const float2 *tw, float2 *out, long nblocks, bool fused, hipStream_t s)
{
    return launch_v4_t<127, 5, 2, 8, false, true, true>((const float2 *)bytes, taps, pal, tw, out, nblocks, fused, s, nullptr); // 3 waves per SIMD: 0.52 against 0.46 ms
}

hipError_t launch_chain_v4_shape_u8(int K, int D, const void *bytes, const float *taps, bool pal, const float2 *tw, float2 *out, long nblocks, bool fused,
                                    hipStream_t s)
{
    const float2 *x = (const float2 *)bytes;
    if (K == 63 && D == 5) return launch_v4_t<63, 5, 2, 8, false, true, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    if (K == 127 && D == 1) return launch_v4_t<127, 1, 2, 8, false, true, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    if (K == 63 && D == 1) return launch_v4_t<63, 1, 2, 8, false, true, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    if (K == 127 && D == 3) return launch_v4_t<127, 3, 2, 8, false, true, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    return hipErrorNotSupported;
}

// the same kernel for the other tap / decimation pairs with a fused build (K - D even, image within the per-wave LDS budget)
hipError_t launch_chain_v4_shape(int K, int D, const float2 *x, const float *taps, bool pal, const float2 *tw, float2 *out, long nblocks, bool fused,
                                 hipStream_t s)
{
    if (K == 63 && D == 5) return launch_v4_t<63, 5, 2, 8, false, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    if (K == 127 && D == 1) return launch_v4_t<127, 1, 2, 8, false, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    if (K == 63 && D == 1) return launch_v4_t<63, 1, 2, 8, false, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    if (K == 127 && D == 3) return launch_v4_t<127, 3, 2, 8, false, true>(x, taps, pal, tw, out, nblocks, fused, s, nullptr);
    return hipErrorNotSupported;
}

template <int K, int D>
static hipError_t launch_v4_list_t(const float2 *const *x, float2 *const *out, const long *nblocks, int count, const float *taps,
                                   bool pal, const float2 *tw, bool fused, hipStream_t s)
{
    ChainList list;
    long total = 0;
    for (int i = 0; i < count; ++i) total += nblocks[i];
    // one rule for the whole launch, from its total: the runs of a list of small messages are as short as those of one message of that size
    const long bpw = chain_v4_blocks_per_wave(total, 2);
    unsigned w = 0;
    for (int i = 0; i < count; ++i) {
        list.x[i] = x[i];
        list.out[i] = out[i];
        list.nblocks[i] = nblocks[i];
        list.wave0[i] = w;
        w += (unsigned)((nblocks[i] + bpw - 1) / bpw);
    }
    list.wave0[count] = w;
    list.count = count;
    constexpr size_t LDS = chain_v4_lds<K, D, 2>(); // the single launch's request: the dispatcher packs no extra wave onto a CU
    if (pal) { // the resident-taps kernel's precondition
        if (fused) hipLaunchKernelGGL((chain_v4_list_kernel<K, D, true>), dim3(w), dim3(64), LDS, s, list, taps, tw, bpw);
        else hipLaunchKernelGGL((chain_v4_list_kernel<K, D, false>), dim3(w), dim3(64), LDS, s, list, taps, tw, bpw);
    } else {
        if (fused) hipLaunchKernelGGL((chain_v4_anytaps_list_kernel<K, D, true>), dim3(w), dim3(64), LDS, s, list, taps, tw, bpw);
        else hipLaunchKernelGGL((chain_v4_anytaps_list_kernel<K, D, false>), dim3(w), dim3(64), LDS, s, list, taps, tw, bpw);
    }
    return hipGetLastError();
}

// count (1 ... REDIO_LIST_MAX) messages of the fused cf32 shapes in one launch: 16-byte aligned inputs, nblocks[i] >= 1 each
// pal: the plan's taps are bit-palindromic (the resident-taps list kernel), else the any-taps twin runs
hipError_t launch_chain_list(int K, long D, const float2 *const *x, float2 *const *out, const long *nblocks, int count, const float *taps,
                             bool pal, const float2 *tw, bool fused, hipStream_t s)
{
    if (count < 1 || count > REDIO_LIST_MAX) return hipErrorInvalidValue;
    for (int i = 0; i < count; ++i)
        if (nblocks[i] < 1 || (reinterpret_cast<uintptr_t>(x[i]) & 15) != 0) return hipErrorInvalidValue;
    if (K == 127 && D == 5) return launch_v4_list_t<127, 5>(x, out, nblocks, count, taps, pal, tw, fused, s);
    if (K == 127 && D == 3) return launch_v4_list_t<127, 3>(x, out, nblocks, count, taps, pal, tw, fused, s);
    if (K == 127 && D == 1) return launch_v4_list_t<127, 1>(x, out, nblocks, count, taps, pal, tw, fused, s);
    if (K == 63 && D == 5) return launch_v4_list_t<63, 5>(x, out, nblocks, count, taps, pal, tw, fused, s);
    if (K == 63 && D == 1) return launch_v4_list_t<63, 1>(x, out, nblocks, count, taps, pal, tw, fused, s);
    return hipErrorNotSupported;
}

// stand-alone decimating FIR on whole 1024-output blocks (16-byte aligned cf32 in and out) for the shapes the chain kernel is
// built for: the chain's data path (wave-private image, halo carried in LDS, register prefetch, taps in SGPRs), storing the
// decimated samples instead of transforming them.  hipErrorNotSupported: no such instantiation (the tiled kernels run).
hipError_t launch_fir_v4(int K, int D, const float2 *x, const float *taps, bool pal, float2 *y, long nblocks, bool fused, hipStream_t s)
{
    // Three wavefronts per SIMD (round 5): without the transform these instantiations need 94-145 registers, and the third wavefront
    // hides more of the window reads' and the stream's latency -- 2^26 samples: 127 / 5 0.1189 -> 0.1109 ms (67.7 -> 72.6 % of 8 TB/s),
    // 63 / 5 0.1007 -> 0.0983, 63 / 1 0.2561 -> 0.2441; 2^28: 0.4901 -> 0.4818, 0.4655 -> 0.4664, 0.9973 -> 0.9688; the reference-rounding
    // builds 4-6 % (profiles/r05_fir_three_waves.txt; interleaved A/B in one process, bit-identical).  REDIO_FIR_WPS2: measurement builds.
    if (!measure_env("REDIO_FIR_WPS2")) {
        if (K == 127 && D == 5) return launch_v4_t<127, 5, 3, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
        if (K == 63 && D == 5) return launch_v4_t<63, 5, 3, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
        if (K == 63 && D == 1) return launch_v4_t<63, 1, 3, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
        if (K == 127 && D == 3) return launch_v4_t<127, 3, 3, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
    }
#ifdef REDIO_MEASURE
    if (K == 127 && D == 5) return launch_v4_t<127, 5, 2, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
    if (K == 63 && D == 5) return launch_v4_t<63, 5, 2, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
    if (K == 63 && D == 1) return launch_v4_t<63, 1, 2, 8, true>(x, taps, pal, nullptr, y, nblocks, fused, s, nullptr);
#endif
    // (127 taps, no decimation: VALU-bound, and the 256-thread tiled kernel with 8 outputs per lane is faster -- 0.44 against 0.56 ms per 2^26 samples;
    //  127 taps / 3 runs here since round 5 with three wavefronts per SIMD: 0.1589 against the chunked tiled kernel's 0.1713 ms, profiles/r05_fir_mid_shapes.txt)
    return hipErrorNotSupported;
}

} // namespace redio
