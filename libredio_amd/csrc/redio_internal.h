// redio_internal.h -- launch entry points shared between the kernel files and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/redio.h"
#include "fft_core.h"
#include "fft_route.h"

// ---- host helpers of every *_api / plan file: the error mapping, the early return, "is this stream capturing", scratch growth ----
static inline int hip_rc(hipError_t e) { return e == hipSuccess ? REDIO_OK : REDIO_ERR_HIP_BASE - (int)e; }
#define REDIO_TRY(expr)                          \
    do {                                         \
        hipError_t _e = (expr);                  \
        if (_e != hipSuccess) return hip_rc(_e); \
    } while (0)

namespace redio {

#pragma GCC visibility push(hidden) // library-internal: not in the exported symbol set
// a plan never allocates while its stream is being captured into a graph: it returns REDIO_ERR_NOT_RESERVED instead
inline bool stream_capturing(hipStream_t st)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(st, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// plan-owned scratch of `need` elements of `elem` bytes: nothing if it is large enough, else free, redio_malloc, and the new
// capacity only once the allocation succeeded
inline int scratch_grow(void **p, size_t *cap, size_t need, size_t elem)
{
    if (need <= *cap) return REDIO_OK;
    if (int rc = redio_free(*p)) return rc;
    *p = nullptr; *cap = 0;
    if (int rc = redio_malloc(p, need * elem)) return rc;
    *cap = need;
    return REDIO_OK;
}
#pragma GCC visibility pop

// Launch-geometry knobs for measurement (tools/ablate.sh, tools/chain_variants.py ...): read from the environment ONLY in a
// -DREDIO_MEASURE build (make EXTRA=-DREDIO_MEASURE OUT=../_build_measure).  The shipped library reads no environment variable.
#ifdef REDIO_MEASURE
inline const char *measure_env(const char *name) { return getenv(name); }
#else
inline const char *measure_env(const char *) { return nullptr; }
#endif

// The FIR and chain plans decide ONCE, at creation, whether their taps are bit-palindromic: taps[i] and taps[K-1-i] the same 32-bit
// pattern for every i (+0.0 against -0.0, or a NaN against anything else, is not).  The chain-form kernels (chain_v4.hip) keep such
// taps resident in scalar registers; every launcher that can reach them takes the answer as `taps_pal`.
inline bool taps_bit_palindromic(const float *taps, size_t K)
{
    for (size_t i = 0; i < K / 2; ++i)
        if (memcmp(&taps[i], &taps[K - 1 - i], sizeof(float)) != 0) return false;
    return true;
}

// fir_kernels.hip
hipError_t launch_fir(const void *x, long n_in, const float *taps, bool taps_pal, int K, long D, void *y, long n_out,
                      bool cplx, bool fused, hipStream_t s);

// ddc_kernels.hip: the tuner (oscillator mix fused into the FIR tile load).  x: n_in cf32 samples or, with u8, their interleaved I/Q
// bytes; tab: period L entries extended by DDC_TABLE_EXT (ddc_core.h); first_mod = first_index mod L; y: n_out outputs
hipError_t launch_ddc(const void *x, bool u8, long n_in, unsigned first_mod, const float2 *tab, unsigned L, const float *taps, int K, long D, float2 *y,
                      long n_out, bool fused, hipStream_t s);

// upfirdn_kernels.hip: the rational resampler.  x: n_in samples (f32, or cf32 with cplx); ph / taps: the plan's phase table and polyphase
// taps (upfirdn_core.h) for K taps, up U, down D; y: n_out outputs, each with its whole window inside the n_in samples
struct UpfirdnPhase;
hipError_t launch_upfirdn(const void *x, long n_in, const UpfirdnPhase *ph, const float *taps, long K, long U, long D, void *y, long n_out, bool cplx,
                          bool fused, hipStream_t s);

// ddc_upfirdn_kernels.hip: the tuned resampler (the tuner's mix fused into the resampler's tile load).  x, tab, first_mod as launch_ddc's;
// ph, taps, K, U, D, y, n_out as launch_upfirdn's, the outputs cf32
hipError_t launch_ddc_upfirdn(const void *x, bool u8, long n_in, unsigned first_mod, const float2 *tab, unsigned L, const UpfirdnPhase *ph, const float *taps,
                              long K, long U, long D, float2 *y, long n_out, bool fused, hipStream_t s);

// fft_kernels.hip
constexpr int FFT_MAX_STAGES = 32;
struct FftPlanDev {
    int nfft;
    int inverse;
    int nstages;
    FftStage st[FFT_MAX_STAGES];
    const float2 *tw;     // device twiddle table, nfft entries
    const float2 *tw_pass; // powers of two from 32768 up: the same values re-ordered per pass (fftbig_tables_*), else null
    const int *leaf_src;  // device table: leaf position -> input index (digit reversal), nfft entries
    const int *leaf_pos;  // the inverse: input index -> leaf position
    unsigned magic_m[FFT_MAX_STAGES]; // ceil(2^32 / m) per stage and ceil(2^32 / nfft): exact quotients by __umulhi for
    unsigned magic_n;                 // dividends below 2^16 * ... (b * m < 2^32), which LDS-resident sizes satisfy
};
// per-pass twiddle tables of the multi-pass transforms: element count for nfft (0: none needed) and the device-side build
size_t fftbig_tables_elems(int nfft);
hipError_t fftbig_tables_build(const float2 *tw, float2 *tables, int nfft, hipStream_t s);
// the route of the plan (fft_route.h) decides the kernels.  A route without in_place_ok wants in != out, one with
// needs_work wants work (nfft * nbatch float2): hipErrorInvalidValue otherwise -- the C-ABI layer stages such calls before it
// launches.  hipErrorNotSupported: no kernel for this plan
hipError_t launch_fft(const FftPlanDev &p, const float2 *in, float2 *out, long nbatch, hipStream_t s, long in_stride = 0,
                      float2 *work = nullptr);
// the forward one-wave transforms (2048, 4096) with u8 I/Q bytes in: in holds one 16-bit word per sample (2-byte aligned), transform xf
// starts at in + xf in_stride, win is null or nfft values multiplied in after the conversion; hipErrorNotSupported for every other plan
bool fft_u8_supported(const FftPlanDev &p);
hipError_t launch_fft_u8(const FftPlanDev &p, const uint16_t *in, const float *win, float2 *out, long nbatch, long in_stride, hipStream_t s);
#pragma GCC visibility push(hidden)
template <int N> // fft_ct.h, instantiated for the sizes of REDIO_FFT_CT_SIZES by fft_ct_lo.hip / fft_ct_hi.hip
hipError_t launch_fft_ct(const FftPlanDev &p, const float2 *in, float2 *out, long nbatch, long in_stride, bool inv, hipStream_t s);
#pragma GCC visibility pop
// one launch over a list of count (1 ... REDIO_LIST_MAX) messages of nbatch[i] >= 1 consecutive transforms each; nfft 1024 only
hipError_t launch_fft1k_list(const FftPlanDev &p, const float2 *const *in, float2 *const *out, const long *nbatch, int count, hipStream_t s);

// fftr_kernels.hip: the real-input transform.  launch_fftr1k: 2048 real points per row fused into the one-wave 1024-point transform
// (tw: the complex plan's table, stw: the M / 2 super twiddles; strides in elements of their own side).  launch_fftr_split: the
// split pass of every other size, Z -> freq (forward) or freq -> T (inverse), strides in cf32
hipError_t launch_fftr1k(bool inverse, const void *in, void *out, const float2 *tw, const float2 *stw, long nbatch, long in_stride,
                         long out_stride, hipStream_t s);
hipError_t launch_fftr_split(bool inverse, const float2 *src, long src_stride, float2 *dst, long dst_stride, const float2 *stw, int M, long nbatch,
                             hipStream_t s);

// ovsave_real_kernels.hip: overlap-save on real streams.  launch_ovsave_real2k: 2048-sample blocks, one kernel (tw_*: the 1024-point
// complex tables, stw_*: the super twiddles of the forward / inverse real plans, Hc: 1025 bins; x 4-byte, out 8-byte aligned, hop even).
// The others are the product, conjugate, scaled-copy and row-gather passes of the generic path (ovsave_real_api.hip).
hipError_t launch_ovsave_real2k(const float *x, long hop, const float2 *tw_f, const float2 *tw_i, const float2 *stw_f, const float2 *stw_i,
                                const float2 *Hc, float *out, long nblk, float scale, hipStream_t s);
hipError_t launch_ovsave_real_mul(float2 *S, const float2 *Hc, long nblk, int nbins, hipStream_t s);
hipError_t launch_ovsave_real_conj(float2 *H, int nbins, hipStream_t s);
hipError_t launch_ovsave_real_scale_out(const float *y, float *out, long nblk, long nfft, long hop, float scale, hipStream_t s);
hipError_t launch_ovsave_real_rows(const float *x, float *rows, long nblk, long nfft, long hop, hipStream_t s);

// pspec_kernels.hip: the integrated power spectrum.  launch_pspec1k: 1024-point transforms, one wavefront per unit (a row of K
// transforms, or with `split` one segment of at most 16); dst: 1024 f32 per unit; win: 1024 values or null; tw: the plan's forward table.
// The others are the generic path's row gather, the accumulate pass over segments [q0, q0 + nseg) of the call (spec: the spectrum of
// transform g_base; dst: N f32 per segment of the call) and the fold of S partials per row (pspec_api.hip).
hipError_t launch_pspec1k(const float2 *x, long step, long K, const float *win, const float2 *tw, float *dst, long nunits, bool split, hipStream_t s);
hipError_t launch_pspec_rows(const float2 *x, const float *win, float2 *rows, long ntr, long N, long step, hipStream_t s);
// the two entry kernels on u8 I/Q bytes: x holds one 16-bit word per sample (2-byte aligned)
hipError_t launch_pspec1k_u8(const uint16_t *x, long step, long K, const float *win, const float2 *tw, float *dst, long nunits, bool split, hipStream_t s);
hipError_t launch_pspec_rows_u8(const uint16_t *x, const float *win, float2 *rows, long ntr, long N, long step, hipStream_t s);
hipError_t launch_pspec_accum(const float2 *spec, float *dst, long q0, long nseg, long N, long K, long g_base, hipStream_t s);
hipError_t launch_pspec_fold(const float *part, float *out, long nrows, long N, long S, hipStream_t s);

// pfb_pspec_kernels.hip: the fused 64-channel polyphase spectrometer (taps_per_branch 4, 8 or 16).  x: cf32 samples, or with in_u8 one
// 16-bit word per sample (2-byte aligned); nunits: output rows of K channelizer rows each, or with `split` their segments (every segment
// of a whole number of rows); dst: 64 f32 per unit; h, tw64: the channelizer's branch taps and 64-point table.
hipError_t launch_pfbspec64(const void *x, bool in_u8, const float *h, const float2 *tw64, float *dst, long nunits, long K, int taps_per_branch,
                            bool split, bool fused, hipStream_t s);

// pfb_pspec_p2.hip: the same in the workgroup form of pfb_p2_kernel, for the shapes of pfb_p2_supported() (32, 128, 256, 512 or 1024
// channels x 4, 8 or 16 taps per branch; hipErrorNotSupported otherwise).  dst: nchan f32 per unit; tw: the nchan-entry forward table;
// Tord: the 512-point plan's stage-ordered copy (512 channels only).  The stream geometry is pfb_pspec_p2_core.h's.
bool pfb_p2_supported(int nchan, int taps_per_branch); // pfb_p2.hip
hipError_t launch_pfbspec_p2(const void *x, bool in_u8, const float *h, const float2 *tw, const float2 *Tord, float *dst, long nunits, long K, int nchan,
                             int taps_per_branch, bool split, bool fused, hipStream_t s);

// pspec_real_kernels.hip: the real-input integrated power spectrum.  launch_pspecr2k: 2048 real points per transform, one wavefront per
// unit (a row of K transforms, or with `split` one segment of at most 16); x: 4-byte aligned; dst: 1025 f32 per unit; win: 2048 values
// or null; tw / stw: the tables of the plan's redio_fftr.  launch_pspec_real_rows: the generic path's row gather (rows: ntr packed
// rows of N f32); its accumulate and fold passes are launch_pspec_accum / launch_pspec_fold with a row of N / 2 + 1 bins.
hipError_t launch_pspecr2k(const float *x, long step, long K, const float *win, const float2 *tw, const float2 *stw, float *dst, long nunits,
                           bool split, hipStream_t s);
hipError_t launch_pspec_real_rows(const float *x, const float *win, float *rows, long ntr, long N, long step, hipStream_t s);

// overlap-save at nfft 1024 (one wave per block) and 4096: one kernel, no work buffers; at 4096 / 16384 tw_f / tw_i (4096) and
// Tf / Ti (16384) are the plans' stage-ordered twiddle copies (redio_fft_twiddles_pass_dev)
hipError_t launch_ovsave1k(const float2 *x, long hop, const float2 *tw_f, const float2 *tw_i, const float2 *Hc, float2 *out, long nblk,
                           float scale, hipStream_t s);
hipError_t launch_ovsave2k(const float2 *x, long hop, const float2 *Tf, const float2 *Ti, const float2 *Hc, float2 *out, long nblk,
                           float scale, hipStream_t s); // 2048-point blocks, the same scheme
hipError_t launch_ovsave8k(const float2 *x, long hop, const float2 *Tf, const float2 *Ti, const float2 *Hc, float2 *out, long nblk,
                           float scale, hipStream_t s); // 8192-point blocks: four waves per block
hipError_t launch_ovsave4k(const float2 *x, long hop, const float2 *tw_f, const float2 *tw_i, const float2 *Hc, float2 *out, long nblk,
                           float scale, hipStream_t s);
hipError_t launch_ovsave16k(const float2 *x, long hop, const float2 *tw_f, const float2 *tw_i, const float2 *Tf, const float2 *Ti, const float2 *Hc,
                            float2 *out, long nblk, float scale, hipStream_t s); // the same at nfft 16384
// overlap-save at nfft 65536: x (block b at x + b*hop) -> out (hop valid samples per block), work buffers a, b of `chunk` blocks each
// (doubled: two chunks each -- the three passes of consecutive chunks then share one launch per step)
hipError_t launch_ovsave64k(const float2 *x, long hop, float2 *a, float2 *b, const float2 *tw_f, const float2 *tw_i, const float2 *Tf,
                            const float2 *Ti, const float2 *Hc, float2 *out, long nblk, long chunk, float scale, hipStream_t s, bool doubled);

// chain_kernels.hip : FIR(K taps, decimate D) -> nfft-point forward transform, fused
bool chain_supported(int K, long D, int nfft);
hipError_t launch_chain_u8(const FftPlanDev &p, const void *bytes, const float *taps, bool taps_pal, int K, long D, float2 *out, long nblocks, bool fused,
                           hipStream_t s);
hipError_t launch_chain(const FftPlanDev &p, const float2 *x, long n_in, const float *taps, bool taps_pal, int K, long D,
                        float2 *out, long nblocks, bool fused, hipStream_t s, unsigned long long *dbg = nullptr, long dbg_cap = 0);
// chain_v4.hip: one launch over a list of count (1 ... REDIO_LIST_MAX) messages of the fused cf32 shapes, 16-byte aligned inputs,
// nblocks[i] >= 1 each (hipErrorNotSupported: no such shape)
hipError_t launch_chain_list(int K, long D, const float2 *const *x, float2 *const *out, const long *nblocks, int count, const float *taps,
                             bool taps_pal, const float2 *tw, bool fused, hipStream_t s);
long chain_v4_blocks_per_wave(long nblocks, int WPS = 2); // chain_v4.hip: consecutive blocks one wavefront of the fused kernel owns (WPS wavefronts per SIMD: the chain 2, the FIR alone 3)
// the fused kernel's name as rocprofv3 prints it (spaces removed), so that a counter file can be tied to the kernel a plan launches
const char *chain_kernel_name(int K, long D, bool fused_math, bool taps_pal, char *buf, size_t cap);

// misc_kernels.hip
hipError_t launch_synth_iq(float2 *out, uint32_t seed, uint64_t first, long n, hipStream_t s);
hipError_t launch_synth_f32(float *out, uint32_t seed, uint64_t first, long n, hipStream_t s);

// overlap-save with a block size of the multi-pass transform family (32768, 131072 ...): six passes
bool ovsave_big_size(int nfft);
hipError_t launch_ovsave_big(const FftPlanDev &fw, const FftPlanDev &bw, const float2 *x, long hop, float2 *a, float2 *b, const float2 *Hc,
                             float2 *out, long nblk, float scale, hipStream_t s);
// CU count of the device the calling thread is bound to (kept per device: a process may drive several GPUs)
inline int num_cus()
{
    static int cus[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cus[dev]) {
        hipDeviceProp_t prop;
        int n = 0;
        if (hipGetDeviceProperties(&prop, dev) == hipSuccess) n = prop.multiProcessorCount;
        cus[dev] = n > 0 ? n : 256;
    }
    return cus[dev];
}

} // namespace redio

// plan shapes for the carried-history layer (stream_carry.hip); defined next to each plan struct
struct redio_fir; struct redio_chain; struct redio_pfb; struct redio_ovsave; struct redio_ovsave_real; struct redio_pspec; struct redio_pspec_real; struct redio_pfb_pspec; struct redio_ddc; struct redio_upfirdn; struct redio_pfb_synth; struct redio_ddc_upfirdn; struct redio_pfb_os; struct redio_pfb_os_synth;
void redio_upfirdn_shape(const redio_upfirdn *h, size_t *period_out, size_t *period_in, size_t *window, unsigned *flags, int *device);
// redio_upfirdn_enqueue for the carried-history layer: exactly `periods` periods (periods * period_out outputs) from n_in samples
int redio_upfirdn_enqueue_periods(redio_upfirdn *h, const void *d_in, size_t n_in, size_t periods, void *d_out, void *stream);
void redio_ddc_shape(const redio_ddc *h, size_t *ntaps, size_t *decim, int *device);
void redio_ddc_upfirdn_shape(const redio_ddc_upfirdn *h, size_t *period_out, size_t *period_in, size_t *window, int *device);
// redio_ddc_upfirdn_enqueue[_u8] for the carried-history layer: exactly `periods` periods from n_in samples (u8: 2 * n_in bytes)
int redio_ddc_upfirdn_enqueue_periods(redio_ddc_upfirdn *h, const void *d_in, size_t n_in, bool u8, size_t periods, uint64_t first_index, void *d_out,
                                      void *stream);
void redio_fir_shape(const redio_fir *h, size_t *ntaps, size_t *decim, unsigned *flags, int *device);
void redio_chain_shape(const redio_chain *h, size_t *ntaps, size_t *decim, int *nfft, int *device);
void redio_pfb_shape(const redio_pfb *h, int *nchan, int *taps_per_branch, int *device);
void redio_pfb_synth_shape(const redio_pfb_synth *h, int *nchan, int *taps_per_branch, int *device);
void redio_pfb_os_shape(const redio_pfb_os *h, int *nchan, int *taps_per_branch, size_t *hop, int *device);
void redio_pfb_os_synth_shape(const redio_pfb_os_synth *h, int *nchan, int *taps_per_branch, size_t *hop, int *device);
void redio_ovsave_shape(const redio_ovsave *h, int *nfft, size_t *hop, int *device);
void redio_ovsave_real_shape(const redio_ovsave_real *h, int *nfft, size_t *hop, int *device);
void redio_pspec_shape(const redio_pspec *h, int *nfft, size_t *integrate, size_t *step, int *device);
void redio_pspec_real_shape(const redio_pspec_real *h, int *nfft, size_t *integrate, size_t *step, int *device);
void redio_pfb_pspec_shape(const redio_pfb_pspec *h, int *window, size_t *integrate, size_t *step, int *device); // window = nchan * taps_per_branch samples, step = nchan
void redio_pfb_tables(const redio_pfb *h, const float **d_taps, const float2 **d_tw, unsigned *flags, int *fused_kernel); // pfb_api.hip
const float2 *redio_pfb_twiddles_pass(const redio_pfb *h); // pfb_api.hip: what launch_pfb_p2 takes as Tord (512 channels), else null
// redio_ovsave_real_enqueue for the carried-history layer: d_in may be only 4-byte aligned (a message that started on an odd sample)
int redio_ovsave_real_enqueue_any(redio_ovsave_real *h, const void *d_in, size_t n_in, void *d_out, void *stream);

// redio_api.hip: the device twiddle table behind a public FFT handle (library-internal)
struct redio_fft;
// whether a call on this plan goes through its staging buffer (in_place: with d_in == d_out).  A plan that owns a redio_fft and must
// work under graph capture asks here, once, whether its own *_reserve has to call redio_fft_reserve
__attribute__((visibility("hidden"))) bool redio_fft_stages(const redio_fft *h, bool in_place);
const redio::FftPlanDev *redio_fft_plan_dev(const redio_fft *h);
const float2 *redio_fft_twiddles_dev(const redio_fft *h);
const float2 *redio_fft_twiddles_pass_dev(const redio_fft *h); // the pass-ordered copy (multi-pass sizes), else null

// fftr_api.hip: the tables behind a real-input plan (library-internal): the complex plan's twiddles (size nfft / 2) and the super twiddles
struct redio_fftr;
const float2 *redio_fftr_twiddles_dev(const redio_fftr *h);
const float2 *redio_fftr_super_dev(const redio_fftr *h);
