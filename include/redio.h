/*
 * redio.h -- C ABI of libredio.so, the MI355X (gfx950) engine for LibRedio's per-sample DSP blocks.
 *
 * This is the drop-in boundary of SURVEY.md 8(b): plain pointers and sizes, no C++/torch types.
 * Paths below are relative to the reference tree (ade-ma/LibRedio).
 *
 * Two families of entry points share the same kernels:
 *   (1) host-buffer, synchronous calls that replace what the reference computes per message
 *       (redio_convolve_f32 for dsputils::convolve; kiss_fft.h / samplerate.h for the C symbols the
 *       reference's Rust already binds);
 *   (2) device-resident plans (redio_fir_*, redio_fft_*, redio_chain_*, ...) that take device
 *       pointers and a HIP stream and only launch kernels inside *_enqueue, so a graph of blocks can keep
 *       its streams in HBM.  Throughput numbers use (2).  Scratch: the few paths that need a plan-owned
 *       intermediate (the two-kernel chain, staged FFT sizes) size it with the plan's *_reserve(); an
 *       un-reserved plan grows it on first use (an allocation) and refuses to do so while the stream is
 *       being captured (REDIO_ERR_NOT_RESERVED).  Everything else never allocates or synchronises.
 *
 * Every function returns REDIO_OK (0) or a negative redio error / positive HIP error code mapped by
 * redio_strerror(); nothing aborts or panics (the reference's unwrap()/assert!/panic! sites become
 * error returns -- SURVEY.md 5 "failure detection").
 * Thread safety: distinct handles may be used concurrently from distinct threads; each call binds
 * the handle's device first (the reference runs one OS thread per block, src/ratpak.rs:60-185).
 */
#ifndef REDIO_H
#define REDIO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- errors ---- */
enum {
    REDIO_OK = 0,
    REDIO_ERR_ARG = -1,         /* NULL pointer / zero taps / zero decimation / bad size */
    REDIO_ERR_NOMEM = -2,
    REDIO_ERR_UNSUPPORTED = -3, /* shape has no kernel (documented per function) */
    REDIO_ERR_NO_DEVICE = -4,   /* no HIP device: the product path never falls back to the CPU */
    REDIO_ERR_ASSERT = -5,      /* an assert!() of the reference would have fired (e.g. fc >= 0.5) */
    REDIO_ERR_NOT_RESERVED = -6, /* a plan would have to allocate scratch while its stream is being captured */
    REDIO_ERR_COMM = -7,        /* RCCL: librccl.so not loadable, or a communicator call failed */
    REDIO_ERR_HIP_BASE = -1000  /* -(1000 + hipError_t) */
};
const char *redio_strerror(int code);
const char *redio_version(void);

/* ---- device / memory / stream / event helpers (thin, so non-torch hosts can drive plans) ---- */
int redio_device_count(int *count);
int redio_set_device(int device);
int redio_get_device(int *device); /* the calling thread's current device */
int redio_malloc(void **dptr, size_t bytes);
int redio_free(void *dptr);
int redio_upload(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int redio_download(void *dst_host, const void *src_dev, size_t bytes, void *stream);
int redio_copy(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
/* pinned host memory that kernels can address directly (zero-copy over PCIe): *host is the CPU pointer, *dev the
 * pointer to pass as a device buffer.  For small host-resident messages this saves the two staged copies of
 * redio_upload / redio_download (the kiss_fft drop-in uses it up to 8192 points). */
int redio_host_alloc(void **host, void **dev, size_t bytes);
int redio_host_free(void *host);
int redio_stream_create(void **stream);
int redio_stream_destroy(void *stream);
int redio_stream_sync(void *stream); /* NULL = default stream */
/* writes `value` to the 32-bit word at d_word (device-addressable memory, e.g. the device alias of a redio_host_alloc buffer) when the stream
 * reaches this point: a host thread polling the word sees the work enqueued before it finished, without hipStreamSynchronize */
int redio_stream_signal(void *stream, void *d_word, uint32_t value);
/* Launch graphs for launch-bound pipelines (many small messages): every *_enqueue below only launches
 * kernels on the given stream -- no allocation, no synchronisation -- so a sequence of them can be
 * recorded once between redio_graph_begin/end on a stream created by redio_stream_create and replayed
 * with one submission.  Pointers and sizes are baked in: replay on the same buffers.  Run the sequence
 * once un-captured first: plans size their internal scratch on first use.
 * (redio_src_process synchronises and is not capturable; redio_src_enqueue does not synchronise on its queued path but advances the
 * converter's state with every call, so it is not capturable either and returns REDIO_ERR_UNSUPPORTED on a capturing stream;
 * redio_*_create / *_destroy never are.) */
typedef struct redio_graph redio_graph;
int redio_graph_begin(void *stream);
int redio_graph_end(void *stream, redio_graph **g);
int redio_graph_launch(redio_graph *g, void *stream);
int redio_graph_destroy(redio_graph *g);
int redio_event_create(void **event);
int redio_event_destroy(void *event);
int redio_event_record(void *event, void *stream);
int redio_event_elapsed_ms(void *start, void *stop, float *ms); /* synchronises on stop */
/* Ordering between the streams of different blocks without the host: an event for synchronisation only (no time stamps: cheaper to
 * record than redio_event_create's), the wait a consumer's stream performs on the event its producer recorded (work enqueued on `stream`
 * after this call runs after everything the producer's stream held when it recorded `event`; returns at once, nothing blocks the
 * host), and the host-side wait for the places that really hand data to the CPU.  include/kpn_dev.hpp carries such an event in every
 * message (the reference's channels order host Vecs, src/kpn/src/kpn.rs:11; on the device the event is that order). */
int redio_event_create_sync(void **event);
int redio_stream_wait_event(void *stream, void *event);
int redio_event_sync(void *event);
/* device allocations made through redio_malloc since the library was loaded (all threads): lets a host check that a steady-state
 * graph no longer allocates (tests/test_kpn_cpp.py: a bounded ring never allocates after warm-up) */
unsigned long long redio_malloc_count(void);

/* ---- tap generators: src/dsputils/src/dsputils.rs:38-94 (host side, run once per filter) ----
 * Quirk-faithful to the reference as written (window() returns m+1 values, lpf()[1] is NaN, ...);
 * redio_lpf_corrected is the documented-deviation designer used for benchmark taps. */
int redio_window(size_t m, float *out /* m+1 */);                 /* :38-51 */
int redio_sinc(size_t m, float fc, float *out /* m */);           /* :53-63; fc>=0.5 -> REDIO_ERR_ASSERT */
int redio_lpf(size_t m, float fc, float *out);                    /* :66-71 */
int redio_hpf(size_t m, float fc, float *out);                    /* :74-79; m<2 -> REDIO_ERR_ASSERT */
int redio_bsf(size_t m, float fc1, float fc2, float *out);        /* :82-88 */
int redio_bpf(size_t m, float fc1, float fc2, float *out);        /* :91-94 */
int redio_lpf_corrected(size_t m, float fc, float *out);

/* ---- A1: dsputils::convolve, src/dsputils/src/dsputils.rs:30-32 ----
 * Host buffers in/out, synchronous: out[i] = sum_j u[i+j]*v[j] folded left to right from 0.0 with a
 * separately rounded multiply and add (bit-exact with the reference fold).  *nout = nu-nv+1, or 0
 * when nu < nv (windows() yields nothing); nv == 0 -> REDIO_ERR_ASSERT (windows(0) panics). */
int redio_convolve_f32(const float *u, size_t nu, const float *v, size_t nv, float *out, size_t *nout);

/* ---- device-resident FIR plan (A1 extended: complex input x real taps, decimation) ---- */
enum {
    REDIO_FIR_COMPLEX = 1u, /* input/output are interleaved cf32 {re, im}; taps stay real */
    REDIO_FIR_FUSED = 2u    /* acc = fmaf(x, h, acc) instead of acc + x*h: faster, still strict order */
};
typedef struct redio_fir redio_fir;
int redio_fir_create(redio_fir **h, const float *taps_host, size_t ntaps, size_t decim, unsigned flags);
int redio_fir_destroy(redio_fir *h);
/* number of outputs for n_in inputs: 0 if n_in < ntaps, else (n_in - ntaps)/decim + 1 */
size_t redio_fir_nout(const redio_fir *h, size_t n_in);
/* valid-mode over one device buffer; d_out must hold redio_fir_nout() samples; in != out */
int redio_fir_enqueue(redio_fir *h, const void *d_in, size_t n_in, void *d_out, void *stream);

/* ---- the tuner: a frequency-translating FIR (A1c) ----
 * kpn::mul_vecs (src/kpn/src/kpn.rs:198-203) by a periodic constant vector w of `period` cf32 entries, then dsputils::convolve
 * (src/dsputils/src/dsputils.rs:30-32) with decimation, in ONE kernel: the oscillator mix happens while the FIR tile is staged.
 *     m[n] = (xr*wr - xi*wi, xr*wi + xi*wr) with w = osc[(first_index + n) mod period], every operation rounded on its own
 *     y[i] = redio_fir's fold over m[i*decim + j] * taps[j]   (REDIO_FIR_FUSED selects fmaf for the FOLD only; the mix is never contracted)
 * so every output is bit-equal to redio_fir_enqueue (complex) on redio_mul_c32(x, the table tiled from first_index); the u8 entry
 * converts each byte as redio_data_to_samples does (rtlsdr.rs:159-162) before the mix.  first_index is the stream index of the
 * call's sample 0.  redio_osc_table fills a table for the shift num/den of the sample rate (kpn.rs:198-203's constant vector;
 * dsputils.rs:30-32 is untouched by it): period = den / gcd(|num|, den) entries, entry n = exp(2 pi i k / den) with
 * k = (num n) mod den in [0, den), computed in double and cast once, the quarter turns exact (an fs/4 shift multiplies by 1, i, -1, -i);
 * a negative num tunes down; out_c32 == NULL only returns the period; den == 0 or a period above REDIO_DDC_MAX_PERIOD -> REDIO_ERR_ARG.
 * create (kpn.rs:198-203, dsputils.rs:30-32): any caller table (mul_vecs' general c); table and taps are uploaded here.  NULL h /
 *   table / taps, period == 0 or above REDIO_DDC_MAX_PERIOD, ntaps == 0, decim == 0 -> REDIO_ERR_ARG.  flags: REDIO_FIR_FUSED or 0.
 * nout: redio_fir_nout's formula.  route: 1 the specialised tiled kernel (127 / 63 taps at decimation 5 / 1), 2 the any-taps chunked
 *   one (decimation 1, 2, 3, 4, 5, 8, 10), 3 the direct one; 0 for NULL.
 * enqueue / enqueue_u8 (kpn.rs:198-203, dsputils.rs:30-32; nbytes / 2 samples): launch only -- no allocation, no synchronisation, so
 *   capturable.  NULL handle, odd nbytes, NULL or overlapping buffers (in != out) -> REDIO_ERR_ARG; fewer than ntaps samples ->
 *   REDIO_OK, no launch.  Any whole-sample alignment of d_in / d_out and any byte alignment of d_bytes is taken; 16-byte aligned
 *   cf32 (4-byte aligned bytes) run the two-samples-per-load path. */
#define REDIO_DDC_MAX_PERIOD 65536 /* a 512 KiB table */
typedef struct redio_ddc redio_ddc;
int redio_osc_table(long long num, unsigned long long den, float *out_c32, size_t *period);
int redio_ddc_create(redio_ddc **h, const float *osc_host_c32, size_t period, const float *taps_host, size_t ntaps, size_t decim, unsigned flags);
int redio_ddc_destroy(redio_ddc *h);
size_t redio_ddc_nout(const redio_ddc *h, size_t n_in);
size_t redio_ddc_period(const redio_ddc *h);
int redio_ddc_route(const redio_ddc *h);
int redio_ddc_enqueue(redio_ddc *h, const void *d_in_c32, size_t n_in, uint64_t first_index, void *d_out_c32, void *stream);
int redio_ddc_enqueue_u8(redio_ddc *h, const void *d_bytes, size_t nbytes, uint64_t first_index, void *d_out_c32, void *stream);

/* ---- the rational resampler: up by `up`, FIR, down by `down`, as a polyphase FIR (A1d) ----
 * dsputils::convolve (src/dsputils/src/dsputils.rs:30-32) with decimation over the stream z that holds up - 1 zeros behind EVERY sample
 * (z[m up] = x[m], length n up), run on the original samples with every up-th tap -- a stated design, defined as
 *     y[i] = acc after: acc = +0; for j = 0 .. ntaps-1 ascending, ONLY where (i down + j) mod up == 0:
 *                acc = mac(x[(i down + j) / up], taps[j], acc)
 *     mac is redio_fir's: a rounded multiply then a rounded add, or fmaf with REDIO_FIR_FUSED
 *     nout(n) = 0 when n up < ntaps, else (n up - ntaps) / down + 1
 * Positions that hold a stuffed zero are SKIPPED, not multiplied (redio_fir on a zero-stuffed buffer gives the same bits except for
 * the sign of a zero where every earlier product underflows under fmaf, and wherever 0 * inf would appear).  Phase by phase, with
 * g = gcd(up, down), U' = up / g, D' = down / g and r in [0, U'): y[r + U' q] is redio_fir's fold of x[s(r) + q D' + t] * taps[j0 + up t]
 * with j0 = (-(r down)) mod up and s(r) = (r down + j0) / up.  One period is U' outputs from D' new samples and reads the window
 * Wp = ((U' - 1) down + ntaps - 1) / up + 1 samples.  Samples are f32, or cf32 with REDIO_FIR_COMPLEX; the taps stay real.
 * create (dsputils.rs:30-32): the taps are uploaded in polyphase order, one zero-padded sub-filter per phase, with a per-phase table.
 *   flags: REDIO_FIR_COMPLEX, REDIO_FIR_FUSED, with redio_fir_create's meaning.  NULL h / taps, ntaps == 0, up == 0, down == 0 ->
 *   REDIO_ERR_ARG; ntaps > 2^24, up > 65536 or down >= 2^31 -> REDIO_ERR_UNSUPPORTED.
 * nout: the formula above (0 for NULL and for n_in above 2^46, where n_in up would leave 64 bits).  route: 1 the phase-walking tiled kernel (D' in {1, 2, 3, 4, 5, 8, 10}, U' <= 16 and a tile that fits),
 *   2 the direct one; 0 for NULL.  period_out / period_in / window: U', D', Wp (0 for NULL).
 * enqueue (dsputils.rs:30-32, the contract above): launch only -- no allocation, no synchronisation, so capturable; every argument is
 *   checked before anything is launched.  NULL handle, NULL, overlapping or not sample-aligned buffers (in != out) -> REDIO_ERR_ARG;
 *   nout == 0 -> REDIO_OK, no launch.  Any whole-sample alignment is taken: 16-byte aligned buffers run the wide loads and stores, the
 *   other paths give the same bits. */
typedef struct redio_upfirdn redio_upfirdn;
int redio_upfirdn_create(redio_upfirdn **h, const float *taps_host, size_t ntaps, size_t up, size_t down, unsigned flags);
int redio_upfirdn_destroy(redio_upfirdn *h);
size_t redio_upfirdn_nout(const redio_upfirdn *h, size_t n_in);
int redio_upfirdn_route(const redio_upfirdn *h);
size_t redio_upfirdn_period_out(const redio_upfirdn *h);
size_t redio_upfirdn_period_in(const redio_upfirdn *h);
size_t redio_upfirdn_window(const redio_upfirdn *h);
int redio_upfirdn_enqueue(redio_upfirdn *h, const void *d_in, size_t n_in, void *d_out, void *stream);

/* ---- the tuned resampler: the tuner's mix in front of the rational resampler, in one kernel (A1e) ----
 * kpn::mul_vecs (src/kpn/src/kpn.rs:198-203) by a periodic constant vector of `period` cf32 entries, then the polyphase form of
 * dsputils::convolve (src/dsputils/src/dsputils.rs:30-32) that redio_upfirdn_* runs -- tuner -> resampler, the receiver's usual pair,
 * without the mixed stream ever written to memory:
 *     m[n] = (xr*wr - xi*wi, xr*wi + xi*wr) with w = osc[(first_index + n) mod period]   redio_ddc's mix: every operation rounded on
 *                                                                                         its own, never contracted
 *     y    = redio_upfirdn's contract over m   (stuffed zeros skipped; REDIO_FIR_FUSED selects fmaf for the FOLD only)
 *     nout = redio_upfirdn_nout's formula
 * so every output is bit-equal to redio_upfirdn_enqueue (complex) on redio_mul_c32(x, the table tiled from first_index).  Input is cf32,
 * or the receiver's interleaved u8 I/Q bytes, converted as redio_data_to_samples does (rtlsdr.rs:159-162) before the mix; the output is
 * always cf32 and the taps are real.  first_index is the stream index of the call's sample 0.
 * create (kpn.rs:198-203, dsputils.rs:30-32): table and taps are uploaded here, the table as redio_ddc's, the taps in redio_upfirdn's
 *   polyphase order.  flags: REDIO_FIR_FUSED or 0.  NULL h / table / taps, period == 0 or above REDIO_DDC_MAX_PERIOD, ntaps == 0,
 *   up == 0, down == 0 -> REDIO_ERR_ARG; ntaps > 2^24, up > 65536 or down >= 2^31 -> REDIO_ERR_UNSUPPORTED.
 * nout / route / period_out / period_in / window: redio_upfirdn's (the route is decided on the cf32 geometry for both entries);
 *   period: the oscillator's.  All 0 for NULL.
 * enqueue / enqueue_u8 (kpn.rs:198-203, dsputils.rs:30-32; nbytes / 2 samples): launch only -- no allocation, no synchronisation, so
 *   capturable; every argument is checked before anything is launched.  NULL handle, odd nbytes, NULL or overlapping buffers
 *   (in != out), a cf32 pointer that is not 8-byte aligned -> REDIO_ERR_ARG; nout == 0 -> REDIO_OK, no launch.  Bytes are taken at any
 *   alignment; 16-byte aligned cf32 (4-byte aligned bytes) run the two-samples-per-load path, a 16-byte aligned output the wide stores,
 *   the other paths give the same bits. */
typedef struct redio_ddc_upfirdn redio_ddc_upfirdn;
int redio_ddc_upfirdn_create(redio_ddc_upfirdn **h, const float *osc_host_c32, size_t period, const float *taps_host, size_t ntaps, size_t up, size_t down,
                             unsigned flags);
int redio_ddc_upfirdn_destroy(redio_ddc_upfirdn *h);
size_t redio_ddc_upfirdn_nout(const redio_ddc_upfirdn *h, size_t n_in);
int redio_ddc_upfirdn_route(const redio_ddc_upfirdn *h);
size_t redio_ddc_upfirdn_period(const redio_ddc_upfirdn *h);
size_t redio_ddc_upfirdn_period_out(const redio_ddc_upfirdn *h);
size_t redio_ddc_upfirdn_period_in(const redio_ddc_upfirdn *h);
size_t redio_ddc_upfirdn_window(const redio_ddc_upfirdn *h);
int redio_ddc_upfirdn_enqueue(redio_ddc_upfirdn *h, const void *d_in_c32, size_t n_in, uint64_t first_index, void *d_out_c32, void *stream);
int redio_ddc_upfirdn_enqueue_u8(redio_ddc_upfirdn *h, const void *d_bytes, size_t nbytes, uint64_t first_index, void *d_out_c32, void *stream);

/* ---- lists of independent messages for one launch (redio_fft_enqueue_list, redio_chain_enqueue_list) ----
 * The reference runs one kissfft::fft per message of block_size samples (src/kissfft/src/kissfft.rs:20-27 asserts din.len() ==
 * block_size) and one chain per message from a block thread (src/ratpak.rs:60-185); a launch per small message costs a fixed floor
 * (about 10 us).  A list call takes up to REDIO_LIST_MAX such messages -- each with its own input, length and output -- and gives,
 * bit for bit, what `count` single calls in list order give.  `n` is what the single call takes (input samples for the chain,
 * transforms for the FFT); an entry that yields no output is skipped; count > REDIO_LIST_MAX runs as several launches.
 * Preconditions: in != out for every entry (REDIO_ERR_ARG otherwise), and no output overlaps another output or any input of the
 * list (the entries run concurrently).  Every entry is checked before anything is launched. */
#define REDIO_LIST_MAX 32
typedef struct {
    const void *in;
    size_t n; /* what the single call takes */
    void *out;
} redio_msg;

/* ---- A5: kissfft::fft block, src/kissfft/src/kissfft.rs:18-31 (device-resident, batched) ----
 * nbatch consecutive messages of exactly nfft cf32 samples; unnormalised; inverse!=0 flips the sign
 * of the exponent.  Arithmetic order of the published kissfft butterflies (bit-exact with
 * oracle/oracle_kiss.c).  d_in == d_out is allowed. */
typedef struct redio_fft redio_fft;
int redio_fft_create(redio_fft **h, int nfft, int inverse);
int redio_fft_destroy(redio_fft *h);
int redio_fft_enqueue(redio_fft *h, const void *d_in, void *d_out, size_t nbatch, void *stream);
/* staging for the sizes that need it (in-place calls of the multi-launch path, prime factors above 5 beyond LDS) */
int redio_fft_reserve(redio_fft *h, size_t nbatch);
/* messages that start every in_stride samples (overlapping blocks when in_stride < nfft); no aliasing */
int redio_fft_enqueue_strided(redio_fft *h, const void *d_in, void *d_out, size_t nbatch, long in_stride, void *stream);
/* kissfft::fft (kissfft.rs:18-31) over a list: entry i is msgs[i].n consecutive transforms from msgs[i].in to msgs[i].out (list
 * preconditions above).  nfft = 1024 is ONE launch per REDIO_LIST_MAX entries that neither allocates nor synchronises (capturable);
 * every other size runs redio_fft_enqueue per entry -- the same bits, one launch per entry. */
int redio_fft_enqueue_list(redio_fft *h, const redio_msg *msgs, size_t count, void *stream);

/* ---- the real-input transform: kiss_fftr / kiss_fftri of the kissfft library (tools/kiss_fftr.c), device-resident, batched ----
 * The other half of the library kiss_fft.h stands in for; the reference's real streams (dsputils::convolve, samplerate::resample,
 * the magnitudes of rtlsdr / bitfount) get their spectra without widening to cf32.  nfft = N real points, N even; M = N / 2.
 * A forward plan (kiss_fftr) takes nbatch rows of N f32 and writes nbatch rows of M + 1 cf32 (bins 0 ... M; the imaginary parts of
 * bins 0 and M are +0); an inverse plan (kiss_fftri) takes rows of M + 1 cf32 (the imaginary parts of bins 0 and M are ignored) and
 * writes rows of N f32, unnormalised: inverse(forward(x)) = N x.  Arithmetic: the complex transform of size M (redio_fft_*, the same
 * bits) and the published split loop with every multiply and add rounded on its own ("real-input transform").
 * N = 2048 is ONE kernel that moves 8 bytes per real sample and needs no scratch (redio_fftr_is_fused() == 1); every other size runs
 * the complex plan and a split pass through plan-owned scratch (16 bytes per real sample).
 * create: odd nfft or nfft < 2 -> REDIO_ERR_ARG; nfft > 2^25 -> REDIO_ERR_UNSUPPORTED. */
typedef struct redio_fftr redio_fftr;
int redio_fftr_create(redio_fftr **h, int nfft /* real points */, int inverse);
int redio_fftr_destroy(redio_fftr *h);
/* scratch of the generic path for up to nbatch rows per call: afterwards an enqueue of up to nbatch rows neither allocates nor
 * synchronises.  Un-reserved, the scratch grows on first use (REDIO_ERR_NOT_RESERVED while the stream is being captured). */
int redio_fftr_reserve(redio_fftr *h, size_t nbatch);
int redio_fftr_is_fused(const redio_fftr *h);
/* kiss_fftr (forward plan) / kiss_fftri (inverse plan) over nbatch packed rows.  d_in != d_out, both 8-byte aligned;
 * NULL or aliasing pointers -> REDIO_ERR_ARG; nbatch == 0 -> REDIO_OK, no launch. */
int redio_fftr_enqueue(redio_fftr *h, const void *d_in, void *d_out, size_t nbatch, void *stream);
/* the same with row b at d_in + b * in_stride and d_out + b * out_stride, counted in elements of their own side (f32 on the real
 * side, cf32 on the spectrum side).  out_stride >= the output row length; the real-side stride is even (rows stay 8-byte aligned);
 * a forward in_stride < nfft gives overlapping frames (the sliding spectrogram, as redio_fft_enqueue_strided does for complex
 * blocks); in_stride <= 0 or any other stride -> REDIO_ERR_ARG.  An inverse generic-path call with out_stride != nfft is one
 * complex launch per row. */
int redio_fftr_enqueue_strided(redio_fftr *h, const void *d_in, void *d_out, size_t nbatch, long in_stride, long out_stride, void *stream);

/* ---- the integrated power spectrum: |X[k]|^2 of the kissfft::fft block (src/kissfft/src/kissfft.rs:18-31) summed over K transforms ----
 * The transform is the reference's (kissfft.rs:18-31, the bits of redio_fft_*); the integration is NEW -- the reference has no
 * such block -- and is a stated design.  What a spectrum display, a waterfall, a detector or a radiometer reads:
 * the periodogram, or with a window and step < nfft Welch's method.  N = nfft, K = integrate, forward transforms only:
 *     transform t of row r reads x[(r K + t) step ... + N), times window[n] when there is a window (NULL: no multiply at all);
 *     p_t[k] = X[k].re * X[k].re + X[k].im * X[k].im;
 *     segment s of a row holds t in [16 s, min(16 s + 16, K)) (REDIO_PSPEC_SEG): seg_s = ((p_first + p_next) + ...), a left fold in
 *     ascending t;  out[r][k] = ((seg_0 + seg_1) + ...), a left fold in ascending s.  For K <= 16 that is the plain sequential sum.
 * All f32, every multiply and add rounded on its own; the order does not depend on launch geometry.  With W = (K - 1) step + N and
 * H = K step a call of n_in samples gives nrows = (n_in - W) / H + 1 rows (0 when n_in < W; a trailing partial row is dropped) of N
 * f32 in natural bin order, packed.  No fftshift, no dB, no division by sum(w^2): those are the caller's.
 * create: NULL h, nfft < 1, integrate == 0, step == 0 -> REDIO_ERR_ARG; a size redio_fft_create refuses -> its error.
 * N = 1024 is ONE kernel in which the spectra never leave the wave's registers (redio_pspec_is_fused() == 1): 8 N / step bytes read
 *   and 4 / K written per sample.  Every other size gathers (and windows) the rows, runs the plan's own redio_fft and an accumulate
 *   pass through plan-owned scratch in chunks of at most 64 MiB.
 * reserve(h, n_in) sizes the scratch for calls of up to n_in samples (and for redio_pspec_enqueue_spectra calls of as many rows),
 *   after which an enqueue neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED while the
 *   stream is being captured).
 * enqueue: launches only, on the caller's stream.  Fewer than W samples -> REDIO_OK, no launch; NULL or overlapping buffers, d_in
 *   not 8-byte or d_out not 4-byte aligned -> REDIO_ERR_ARG.
 * enqueue_spectra: the same integration over nbatch packed, already transformed rows of N bins (window and step do not apply):
 *   nbatch / K rows come out.  This is how redio_chain_enqueue's spectra are integrated.
 * set_split: 0 auto, 1 one wavefront (or thread group) per whole row, 2 one per segment and a fold pass over the partials.  For tests
 *   and measurement, like redio_chain_set_unfused: the bits are the same in every mode. */
#define REDIO_PSPEC_SEG 16
typedef struct redio_pspec redio_pspec;
int redio_pspec_create(redio_pspec **h, int nfft, size_t integrate, size_t step, const float *window_host /* NULL or nfft */);
int redio_pspec_destroy(redio_pspec *h);
size_t redio_pspec_nrows(const redio_pspec *h, size_t n_in);
int redio_pspec_is_fused(const redio_pspec *h);
int redio_pspec_reserve(redio_pspec *h, size_t n_in);
int redio_pspec_enqueue(redio_pspec *h, const void *d_in_c32, size_t n_in, void *d_out_f32, void *stream);
int redio_pspec_enqueue_spectra(redio_pspec *h, const void *d_spectra_c32, size_t nbatch, void *d_out_f32, void *stream);
int redio_pspec_set_split(redio_pspec *h, int mode);
/* The receiver's own format in: interleaved u8 I/Q bytes (rtlsdr::data_to_samples, src/rtlsdr/src/rtlsdr.rs:159-162) straight into the
 * plan -- nbytes / 2 samples, redio_pspec_nrows(h, nbytes / 2) rows, bit for bit the rows redio_data_to_samples + redio_pspec_enqueue
 * would give on every plan and in every redio_pspec_set_split mode (convert, then the window multiply rounded on its own, then the
 * transform and the blocked sum above).  N = 1024 is ONE kernel that converts at the load: 2 N / step bytes read and 4 / K written per
 * sample, no scratch beyond the segment partials.  At N = 2048 and 4096 the plan's transform converts (and windows) at its own load
 * and writes the spectra into the plan's row scratch; every other size converts inside the row gather into that scratch.  There is
 * never a whole-message cf32 buffer.
 * enqueue_u8: launches only, on the caller's stream; every argument is checked before anything is launched.  Odd nbytes, NULL or
 *   overlapping buffers, d_bytes not 2-byte (a whole sample) or d_out not 4-byte aligned -> REDIO_ERR_ARG; fewer than W samples ->
 *   REDIO_OK, no launch.
 * reserve_u8(h, nbytes) sizes the scratch (the in-place transform's staging included) for u8 calls of up to nbytes bytes, after which
 *   an enqueue_u8 neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED while the stream is
 *   being captured). */
int redio_pspec_enqueue_u8(redio_pspec *h, const void *d_bytes, size_t nbytes, void *d_out_f32, void *stream);
int redio_pspec_reserve_u8(redio_pspec *h, size_t nbytes);

/* ---- the real-input integrated power spectrum: |X[k]|^2 of kiss_fftr (tools/kiss_fftr.c) summed over K transforms of REAL samples ----
 * The power spectrum above for the reference's real f32 streams (the magnitudes of rtlsdr / bitfount, dsputils::convolve,
 * samplerate::resample) without widening them to cf32 and without computing every bin twice.  The transform is kiss_fftr
 * (tools/kiss_fftr.c), the bits of a forward redio_fftr_* plan: the complex transform of size M = N / 2 and the published split
 * loop; the integration is the stated design of DESIGN.md 5.3c, unchanged (the contract of this block: DESIGN.md 5.3d).
 * N = nfft REAL points, even, 2 <= N <= 2^25; K = integrate; B = N / 2 + 1 bins (redio_pspec_real_nbins):
 *     transform t of row r reads x[(r K + t) step ... + N), times window[n] when there is a window (NULL: no multiply at all);
 *     X = kiss_fftr of that row;  p_t[k] = X[k].re * X[k].re + X[k].im * X[k].im for k = 0 ... M (bins 0 and M have imaginary part +0);
 *     segments of REDIO_PSPEC_SEG transforms, a left fold in ascending t inside each, a left fold over them in ascending s.
 * All f32, every multiply and add rounded on its own; the order does not depend on launch geometry.  With W = (K - 1) step + N and
 * H = K step (in real samples) a call of n_in samples gives nrows = (n_in - W) / H + 1 rows (0 when n_in < W; a trailing partial row is
 * dropped) of B f32 in natural bin order, packed -- B is odd at the fused size, so rows are only 4-byte aligned.  No one-sided
 * doubling, no dB, no division by sum(w^2): those are the caller's.
 * create: NULL h, odd nfft, nfft < 2, integrate == 0, step == 0 -> REDIO_ERR_ARG; nfft > 2^25 -> REDIO_ERR_UNSUPPORTED
 *   (redio_fftr_create's ceiling).  The plan owns a forward redio_fftr of size N.
 * N = 2048 is ONE kernel in which the spectra never leave the wave's registers (redio_pspec_real_is_fused() == 1): 4 N / step bytes
 *   read and 4 B / (K step) -- about 2 / K -- written per real sample, half of what the fused redio_fftr alone moves.  Every other
 *   size gathers (and windows) the rows unless the transform can read the caller's buffer (no window, step == N, 8-byte aligned),
 *   runs the plan's own redio_fftr and an accumulate pass through plan-owned scratch in chunks of at most 64 MiB of spectra.
 * reserve(h, n_in) sizes all plan-owned scratch for calls of up to n_in samples (and for enqueue_spectra calls of as many rows), after
 *   which an enqueue neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED while the stream
 *   is being captured).
 * enqueue: launches only, on the caller's stream; every argument is checked before anything is launched.  d_in and d_out are each
 *   4-byte aligned (a real stream has no pair structure: a seam lands on any sample).  NULL or overlapping buffers -> REDIO_ERR_ARG;
 *   fewer than W samples -> REDIO_OK, no launch.
 * enqueue_spectra: the integration alone over nbatch packed rows of B cf32 (redio_fftr_enqueue's output; 8-byte aligned; window and
 *   step do not apply): nbatch / K rows come out.
 * set_split: 0 auto, 1 one wavefront (or thread group) per whole row, 2 one per segment and a fold pass over the partials: the bits
 *   are the same in every mode. */
typedef struct redio_pspec_real redio_pspec_real;
int redio_pspec_real_create(redio_pspec_real **h, int nfft /* real points */, size_t integrate, size_t step, const float *window_host /* NULL or nfft */);
int redio_pspec_real_destroy(redio_pspec_real *h);
size_t redio_pspec_real_nrows(const redio_pspec_real *h, size_t n_in);
size_t redio_pspec_real_nbins(const redio_pspec_real *h); /* nfft / 2 + 1; 0 for NULL */
int redio_pspec_real_is_fused(const redio_pspec_real *h);
int redio_pspec_real_reserve(redio_pspec_real *h, size_t n_in);
int redio_pspec_real_enqueue(redio_pspec_real *h, const void *d_in_f32, size_t n_in, void *d_out_f32, void *stream);
int redio_pspec_real_enqueue_spectra(redio_pspec_real *h, const void *d_spectra_c32, size_t nbatch, void *d_out_f32, void *stream);
int redio_pspec_real_set_split(redio_pspec_real *h, int mode);

/* ---- C2 chain: FIR (ntaps, decimate decim) -> nfft-point forward FFT of consecutive blocks ----
 * Fused single kernel for nfft = 1024 with (ntaps, decim) in {(127, 5), (127, 3), (127, 1), (63, 5), (63, 1)} on a
 * 16-byte aligned stream; other shapes run the FIR and FFT kernels back to back through a plan-owned
 * intermediate buffer (same results).  Trailing decimated
 * samples that do not fill a block are dropped, as kpn::shaper would (src/kpn/src/kpn.rs:278-282). */
typedef struct redio_chain redio_chain;
int redio_chain_create(redio_chain **h, const float *taps_host, size_t ntaps, size_t decim, int nfft, unsigned flags);
int redio_chain_destroy(redio_chain *h);
size_t redio_chain_nblocks(const redio_chain *h, size_t n_in);
int redio_chain_is_fused(const redio_chain *h);
/* force the two-kernel path (for measurement): 0 = fused when available, 1 = never fused */
int redio_chain_set_unfused(redio_chain *h, int unfused);
/* sizes the two-kernel path's intermediate for inputs of up to n_in samples, so that enqueue never allocates */
int redio_chain_reserve(redio_chain *h, size_t n_in);
int redio_chain_enqueue(redio_chain *h, const void *d_in, size_t n_in, void *d_out, void *stream);
/* the chain (dsputils.rs:30-32 -> kissfft.rs:18-31) over a list: entry i is one redio_chain_enqueue of msgs[i].n input samples from
 * msgs[i].in to msgs[i].out (list preconditions above).  A fused plan runs its entries with a 16-byte aligned input as ONE kernel per
 * REDIO_LIST_MAX of them (no allocation, no synchronisation: capturable); the other entries go through redio_chain_enqueue behind it
 * on the same stream.  A two-kernel plan (redio_chain_set_unfused, other shapes) runs redio_chain_enqueue per entry. */
int redio_chain_enqueue_list(redio_chain *h, const redio_msg *msgs, size_t count, void *stream);
/* The receiver's own format in: interleaved u8 I/Q bytes (rtlsdr::data_to_samples, src/rtlsdr/src/rtlsdr.rs:159-162: i as f32 / 127.0 - 1.0)
 * straight into the chain -- nbytes / 2 samples, the spectra redio_data_to_samples + redio_chain_enqueue would give, bit for bit.
 * The shapes with a fused cf32 kernel (above) on 4-byte aligned bytes are ONE kernel ((127, 5): 3.6 bytes per sample through HBM instead
 * of 25.6); other shapes convert
 * into a plan-owned buffer first (grown on first use: REDIO_ERR_NOT_RESERVED inside a stream capture). */
int redio_chain_enqueue_u8(redio_chain *h, const void *d_bytes, size_t nbytes, void *d_out, void *stream);
/* sizes that buffer (and the two-kernel path's intermediate) for messages of up to nbytes bytes, so that enqueue_u8 never allocates */
int redio_chain_reserve_u8(redio_chain *h, size_t nbytes);
/* launch geometry of the fused kernel for a call that yields nblocks blocks (0 for a plan that runs as two kernels): a wavefront
 * owns redio_chain_blocks_per_wave() consecutive blocks (the last one of the launch possibly fewer), the launch has
 * redio_chain_launch_waves() = ceil(nblocks / blocks_per_wave) wavefronts.  Tests pick run boundaries from it, the probes size
 * their stamp buffers from it. */
size_t redio_chain_blocks_per_wave(const redio_chain *h, size_t nblocks);
size_t redio_chain_launch_waves(const redio_chain *h, size_t nblocks);
/* the fused kernel's name as rocprofv3 reports it, spaces removed (e.g. "chain_v4_kernel<127,5,true,2,8,false,true,false,false>"); NULL for a
 * two-kernel plan.  bench.py refuses a counter file (profiles/rNN_traffic.json) recorded for another kernel.  Owned by the plan. */
const char *redio_chain_kernel_name(redio_chain *h);
/* diagnostic, per plan: while d_buf (device memory, capacity_waves records of 4 x u64) is set, wavefront w < capacity_waves of the
 * fused kernel of THIS plan writes {shader cycles, 100 MHz ticks, start tick, XCC/HW id} into record w (tools/clock_probe.py reads
 * the clock the chip holds from it); size it with redio_chain_launch_waves().  NULL (default) turns it off.  Timings of stamped
 * launches are never quoted. */
int redio_chain_set_debug_stamps(redio_chain *h, void *d_buf, size_t capacity_waves);

/* ---- A9: the bit-exact ingest / slicing path of the shipped graph (src/ratpak.rs:60-76) ----
 * All device-resident; results are bit-identical to the reference arithmetic (oracle_bits.c). */
/* rtlsdr::data_to_samples, src/rtlsdr/src/rtlsdr.rs:159-162: byte pairs -> cf32 (i as f32/127.0 - 1.0);
 * an odd byte count is the reference's index panic -> REDIO_ERR_ASSERT */
int redio_data_to_samples(const void *d_bytes, size_t nbytes, void *d_out_c32, void *stream);
/* the |x| map of src/ratpak.rs:64-68: Complex::norm = hypotf(re, im) */
int redio_norm_c32(const void *d_in_c32, size_t n, void *d_out_f32, void *stream);
/* both of the above fused: u8 IQ -> magnitude (2 B read + 4 B written per sample); d_bytes 8-byte and
 * d_mag 16-byte aligned */
int redio_ingest_u8_mag(const void *d_bytes, size_t nbytes, void *d_mag_f32, void *stream);
/* per-block sums in sample order, the `s` of bitfount::trigger (src/bitfount/src/bitfount.rs:48) */
int redio_block_sums(const void *d_in_f32, size_t nblocks, size_t block, void *d_sums_f32, void *stream);
/* bitfount::discretize, src/bitfount/src/bitfount.rs:87-96: max = fold(0.0, f32::max); out = (x > max/2)
 * as one byte per sample (the reference sends usize); d_scratch_u32 holds the max's bit pattern */
int redio_discretize(const void *d_in_f32, size_t n, void *d_out_u8, void *d_scratch_u32, void *stream);
/* bitfount::trigger, src/bitfount/src/bitfount.rs:36-85: state persists across calls; feeds nblocks
 * blocks of `block` f32 magnitudes; emitted buffers are appended to d_out with their lengths in
 * lens[] (host).  Synchronous (the adaptive threshold is a scalar recurrence run on the host).
 * If the buffers this call would emit do not fit (more than lens_cap of them, or more than out_cap
 * floats) nothing is consumed: REDIO_ERR_ARG with the needed counts in *nemit / *total, retry larger. */
typedef struct redio_trigger redio_trigger;
int redio_trigger_create(redio_trigger **h);
int redio_trigger_destroy(redio_trigger *h);
int redio_trigger_feed(redio_trigger *h, const void *d_blocks_f32, size_t nblocks, size_t block, void *d_out_f32, size_t out_cap,
                       size_t *lens, size_t lens_cap, size_t *nemit, size_t *total, void *stream);

/* ---- the run-length / bit-field stage downstream of discretize (src/ratpak.rs:77-119) ----
 * One-byte values (discretize emits 0/1), u64 run lengths, f32 seconds; all device-resident. */
/* kpn::rle, src/kpn/src/kpn.rs:17-29: a run is emitted when the value changes, so the open run is
 * carried in the handle across calls and never flushed.  *nruns runs written (<= cap).  Synchronous. */
typedef struct redio_rle redio_rle;
int redio_rle_create(redio_rle **h);
int redio_rle_destroy(redio_rle *h);
int redio_rle_feed(redio_rle *h, const void *d_in_u8, size_t n, void *d_vals_u8, void *d_counts_u64, size_t cap, size_t *nruns,
                   void *stream);
/* kpn::dle, kpn.rs:32-38: seconds = ct as f32 / s_rate as f32 */
int redio_dle(const void *d_counts_u64, size_t n, size_t s_rate, void *d_seconds_f32, void *stream);
/* kpn::rld, kpn.rs:50-56: (value, count) -> repeated values; d_scratch: (nruns + 1) u64 */
int redio_rld(const void *d_vals_u8, const void *d_counts_u64, size_t nruns, void *d_out_u8, size_t cap, void *d_scratch, size_t *nout,
              void *stream);
/* kpn::dld, kpn.rs:41-47: n = (dur * s_rate) as usize per run; d_scratch: (2 * nruns + 1) u64 */
int redio_dld(const void *d_vals_u8, const void *d_seconds_f32, size_t nruns, float s_rate, void *d_out_u8, size_t cap, void *d_scratch,
              size_t *nout, void *stream);
/* kpn::binconv = eat (kpn.rs:116-124) per message: nmsg messages of nbits one-byte binary digits ->
 * nfields u64 each, MSB first (b2d, kpn.rs:111-113); widths overrunning a message -> REDIO_ERR_ASSERT */
int redio_binconv(const void *d_bits_u8, size_t nmsg, size_t nbits, const size_t *widths, size_t nfields, void *d_out_u64, void *stream);

/* ---- C5: overlap-save FFT convolution (BASELINE.json configs[4]; a new composition) ----
 * The valid-mode correlation of dsputils::convolve (dsputils.rs:30-32) on cf32 with real taps, computed
 * per block of nfft samples: out[b*hop + i] = IFFT(FFT(x[b*hop ..]) .* conj(FFT(taps)))[i] / nfft, i < hop,
 * hop = nfft - ntaps + 1, kissfft-order transforms.  Only whole blocks are produced:
 * nout = ((n_in - nfft)/hop + 1) * hop, 0 when n_in < nfft.  Bit-identical to oracle orc_overlap_save;
 * within K*eps*sum|x*h| of the direct fold. */
typedef struct redio_ovsave redio_ovsave;
int redio_ovsave_create(redio_ovsave **h, const float *taps_host, size_t ntaps, int nfft);
int redio_ovsave_destroy(redio_ovsave *h);
size_t redio_ovsave_nout(const redio_ovsave *h, size_t n_in);
int redio_ovsave_enqueue(redio_ovsave *h, const void *d_in, size_t n_in, void *d_out, void *stream);

/* ---- overlap-save on REAL streams: the same valid-mode correlation (dsputils::convolve is real-only, dsputils.rs:30-32) on f32
 * samples with real taps, through the real-input transforms above (kiss_fftr / kiss_fftri), N = nfft real points per block:
 *     Ke = ntaps | 1 (an even tap count is treated as if one zero tap followed it), hop = N - Ke + 1 -- always even, so every block
 *     starts on an 8-byte boundary;  Hc = conj(kiss_fftr(taps zero-padded to N));
 *     out[b*hop + i] = kiss_fftri(kiss_fftr(x[b*hop .. b*hop + N)) .* Hc)[i] * (1.0f / N), i < hop
 * (product: Y.r = X.r*Hc.r - X.i*Hc.i, Y.i = X.r*Hc.i + X.i*Hc.r, every operation rounded on its own).  Only whole blocks are produced:
 * nout = ((n_in - N)/hop + 1) * hop, 0 when n_in < N.  It moves 4*N/hop + 4 bytes per output sample, half of what redio_ovsave_* moves
 * for the same stream widened to cf32.  Within 2e-6 * sum|taps| * sqrt(log2 N) + 1e-7 of the direct fold.
 * create: taps NULL, ntaps == 0, odd nfft, nfft < 2 or Ke > nfft -> REDIO_ERR_ARG (so ntaps == nfft is refused: nfft - 1
 *   taps at most); nfft > 2^25 -> REDIO_ERR_UNSUPPORTED (redio_fftr_create's ceiling).
 * N = 2048 is ONE kernel without scratch (redio_ovsave_real_is_fused() == 1).  Every other size runs the two transforms, a product
 *   pass and a scaled copy through plan-owned scratch, in chunks of blocks: redio_ovsave_real_reserve(h, n_in) sizes it, after which an
 *   enqueue of up to n_in samples neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED while
 *   the stream is being captured).
 * enqueue: n_in < nfft -> REDIO_OK, no launch; NULL, overlapping or not 8-byte aligned d_in / d_out -> REDIO_ERR_ARG. */
typedef struct redio_ovsave_real redio_ovsave_real;
int redio_ovsave_real_create(redio_ovsave_real **h, const float *taps_host, size_t ntaps, int nfft);
int redio_ovsave_real_destroy(redio_ovsave_real *h);
size_t redio_ovsave_real_nout(const redio_ovsave_real *h, size_t n_in);
int redio_ovsave_real_is_fused(const redio_ovsave_real *h);
int redio_ovsave_real_reserve(redio_ovsave_real *h, size_t n_in);
int redio_ovsave_real_enqueue(redio_ovsave_real *h, const void *d_in_f32, size_t n_in, void *d_out_f32, void *stream);

/* ---- C4: M-channel polyphase channelizer (BASELINE.json configs[3]; a new composition) ----
 * Prototype of nchan*taps_per_branch taps; branch m filters rows x_t[m] = x[nchan*t + m] with
 * g_m[p] = proto[nchan*p + m] using the fold of dsputils::convolve (dsputils.rs:31), then every row
 * goes through kissfft's nchan-point forward transform (kissfft.rs:26).  Output rows: T-P+1 with
 * T = floor(n_in / nchan).  nchan = 64 with taps_per_branch in {4, 8, 16} runs one fused kernel; any other
 * shape runs the branch filters and the nchan-point transform as two passes (same results).
 * flags: REDIO_FIR_FUSED as for redio_fir_create.
 * Output layout: ngroups = 1 -> [row][nchan]; ngroups = G -> [group][row][nchan/G], the send layout
 * of the multi-GPU regrouping (one contiguous chunk per destination rank). */
typedef struct redio_pfb redio_pfb;
int redio_pfb_create(redio_pfb **h, const float *proto_taps_host, int nchan, int taps_per_branch, unsigned flags);
int redio_pfb_destroy(redio_pfb *h);
size_t redio_pfb_nrows(const redio_pfb *h, size_t n_in);
int redio_pfb_enqueue(redio_pfb *h, const void *d_in, size_t n_in, void *d_out, int ngroups, void *stream);
/* the same from the receiver's interleaved u8 I/Q bytes (rtlsdr::data_to_samples, src/rtlsdr/src/rtlsdr.rs:159-162), nbytes / 2 samples,
 * bit for bit the rows of redio_data_to_samples + redio_pfb_enqueue: one kernel for 64 channels x 16 taps per branch (10 instead of
 * 26 bytes per sample through HBM), other shapes convert into a plan-owned buffer first (grown on first use). */
int redio_pfb_enqueue_u8(redio_pfb *h, const void *d_bytes, size_t nbytes, void *d_out, int ngroups, void *stream);
int redio_pfb_reserve_u8(redio_pfb *h, size_t nbytes, int ngroups); /* as redio_pfb_reserve, for messages of up to nbytes bytes */
/* scratch of the two-pass shapes for inputs of up to n_in samples.  The fused 64-channel kernel needs none; the one-kernel shapes (32 ...
 * 1024 channels x 4 / 8 / 16 taps per branch) need it only for an output that is not 16-byte aligned and reserve NOTHING unless
 * REDIO_PFB_RESERVE_TWO_PASS is or-ed into ngroups (un-reserved, that fall-back sizes its scratch at first use and returns
 * REDIO_ERR_NOT_RESERVED inside a capture). */
#define REDIO_PFB_RESERVE_TWO_PASS 0x40000000
int redio_pfb_reserve(redio_pfb *h, size_t n_in, int ngroups);
/* the same as redio_pfb_reserve(h, n_in, ngroups | REDIO_PFB_RESERVE_TWO_PASS) under a name of its own: sizes the two-pass scratch of ANY
 * shape without a fused 64-channel kernel, so that an output that is not 16-byte aligned never allocates (e.g. inside a capture) */
int redio_pfb_reserve_two_pass(redio_pfb *h, size_t n_in, int ngroups);

/* ---- the polyphase spectrometer: |row[c]|^2 of the channelizer's rows summed over K rows (a NEW composition) ----
 * What a waterfall, a detector or a radiometer puts behind a channelizer.  M = nchan, P = taps_per_branch, K = integrate >= 1:
 *     channelizer row t is exactly redio_pfb_enqueue's row t (ngroups = 1): the same branch fold, with or without REDIO_FIR_FUSED,
 *     and the same nchan-point kissfft transform;
 *     p_t[c] = row_t[c].re * row_t[c].re + row_t[c].im * row_t[c].im, every multiply and add rounded on its own;
 *     output row r integrates channelizer rows [r K, r K + K) in the order of the power spectrum above: segments of
 *     REDIO_PSPEC_SEG rows counted from r K, a left fold in ascending t inside each, a left fold over them in ascending s.
 * The order does not depend on launch geometry.  With T = n_in / M a call gives nrows = (T - P + 1) / K rows (0 when T < P + K - 1;
 * a trailing partial row is dropped) of M f32 in natural channel order, packed.  In samples: window W = (K - 1 + P) M, hop H = K M.
 * Bit for bit that is redio_pfb_enqueue followed by redio_pspec_enqueue_spectra of a (nfft = M, integrate = K) plan, for every shape
 * redio_pfb_create accepts -- that composition is the definition -- without the channel rows ever reaching memory on the fused
 * shapes.  No dB, no fftshift, no normalisation: those are the caller's.
 * create: NULL h, integrate == 0 -> REDIO_ERR_ARG; a shape redio_pfb_create refuses -> its error.  flags: as redio_pfb_create, and
 *   REDIO_PFB_PSPEC_BLOCK, which is this plan's own (redio_pfb_create never sees it).
 * redio_pfb_pspec_route() says what a call on the plan runs (0 for NULL):
 *   1  nchan = 64 with taps_per_branch in {4, 8, 16} is ONE kernel, a wavefront per run of rows (redio_pfb_pspec_is_fused() == 1),
 *      from cf32 and from bytes: 8 (or 2) bytes read and 4 / K written per sample, no scratch beyond the segment partials.
 *   2  with REDIO_PFB_PSPEC_BLOCK, nchan in {32, 128, 256, 512, 1024} with taps_per_branch in {4, 8, 16} -- the shapes of the
 *      channelizer's own one-kernel form -- is ONE kernel too, a workgroup per G = max(1, 256 / nchan) runs of rows: the same 8 (or 2)
 *      + 4 / K bytes per sample and no scratch beyond the segment partials.  Opt-in; is_fused() stays 0.  On every other shape the
 *      flag is accepted and changes nothing.
 *   0  every other plan runs its own redio_pfb into plan-owned row scratch in chunks of whole segments with at most 64 MiB of rows, and
 *      an accumulate pass per chunk: 8 read + 8 written + 8 read + 4 / K written per sample.
 * reserve(h, n_in) / reserve_u8(h, nbytes) size all of the scratch, the inner channelizer's included, for calls of up to that many
 *   samples / bytes, after which an enqueue neither allocates nor synchronises; un-reserved it grows on first use
 *   (REDIO_ERR_NOT_RESERVED while the stream is being captured).  On routes 1 and 2 that is the segment partials alone, which only a
 *   call by segments with K > REDIO_PSPEC_SEG touches: every other call there needs no scratch and captures without a reserve.
 * enqueue / enqueue_u8 (interleaved u8 I/Q bytes, rtlsdr.rs:159-162: bit for bit redio_data_to_samples + enqueue): launches only, on
 *   the caller's stream; every argument is checked before anything is launched.  NULL or overlapping buffers, d_in not 8-byte,
 *   d_bytes not 2-byte or d_out not 4-byte aligned, odd nbytes -> REDIO_ERR_ARG; fewer than W samples -> REDIO_OK, no launch.
 * set_split: 0 auto, 1 a wavefront (route 2: a thread group of a workgroup) owns whole output rows, 2 it owns a run of whole segments
 *   and a fold pass finishes: the bits are the same in every mode, on every route and on every device. */
#define REDIO_PFB_PSPEC_BLOCK 4u /* redio_pfb_pspec_create flags: the workgroup kernel (route 2) where the shape has one */
typedef struct redio_pfb_pspec redio_pfb_pspec;
int redio_pfb_pspec_create(redio_pfb_pspec **h, const float *proto_taps_host, int nchan, int taps_per_branch, size_t integrate, unsigned flags);
int redio_pfb_pspec_destroy(redio_pfb_pspec *h);
size_t redio_pfb_pspec_nrows(const redio_pfb_pspec *h, size_t n_in);
int redio_pfb_pspec_is_fused(const redio_pfb_pspec *h);
int redio_pfb_pspec_route(const redio_pfb_pspec *h); /* 0 generic, 1 the 64-channel wave kernel, 2 the workgroup kernel */
int redio_pfb_pspec_reserve(redio_pfb_pspec *h, size_t n_in);
int redio_pfb_pspec_enqueue(redio_pfb_pspec *h, const void *d_in_c32, size_t n_in, void *d_out_f32, void *stream);
int redio_pfb_pspec_enqueue_u8(redio_pfb_pspec *h, const void *d_bytes, size_t nbytes, void *d_out_f32, void *stream);
int redio_pfb_pspec_reserve_u8(redio_pfb_pspec *h, size_t nbytes);
int redio_pfb_pspec_set_split(redio_pfb_pspec *h, int mode);

/* ---- the synthesis filterbank: many narrow channels into one wideband stream (a NEW composition) ----
 * The channelizer is "branch filter, then forward transform".  This is "inverse transform, then the same branch filter".
 * What brings a channelized stream back to one stream after per-channel work, and the transmit direction (a transmultiplexer).
 * M = nchan, P = taps_per_branch; the prototype has M P taps in the channelizer's own layout, g_m[p] = proto[M p + m].  The input is
 * T = n_in / M rows X_t[0 .. M) of cf32 in natural channel order -- redio_pfb_enqueue's ngroups = 1 output layout; a trailing partial
 * row is ignored:
 *     v_t = kissfft's unnormalised M-point INVERSE transform of X_t (kissfft.rs:26 with inv != 0: the bits of an inverse redio_fft);
 *     y[M t + m] = the fold of dsputils::convolve (dsputils.rs:31) over v_{t+p}[m] * g_m[p], from 0.0f in ascending p = 0 .. P - 1:
 *     multiply and add rounded separately, or fmaf with REDIO_FIR_FUSED -- per branch the bits of redio_fir on the column v[:, m].
 * The output is (T - P + 1) M cf32 samples of one stream (0 when T < P); in samples the window is P M and the hop M.  Like every FIR
 * here this is valid-mode correlation with the taps not reversed: for the convolution form pass the prototype with the p order
 * flipped.  There is no 1 / M, as kissfft has none: with one-tap prototypes (1.0 at tap pa on the analysis side, at ps here) the round
 * trip through redio_pfb_enqueue gives M x[i + (pa + ps) M] up to the transforms' rounding.
 * create: NULL h / taps, nchan < 1, taps_per_branch < 1 -> REDIO_ERR_ARG, as redio_pfb_create; a size redio_fft_create refuses ->
 *   its error.  flags: REDIO_FIR_FUSED or 0.
 * redio_pfb_synth_route() says what a call on the plan runs (0 for NULL):
 *   1  nchan = 64 with taps_per_branch in {4, 8, 16} is ONE kernel, a wavefront per run of output rows (is_fused() == 1): 8 bytes read
 *      and 8 written per sample, no scratch; it captures without a reserve.
 *   0  every other plan runs its own inverse redio_fft over the rows into plan-owned scratch and the channelizer's branch pass on the
 *      result, in chunks of at most 64 MiB of rows: 32 bytes per sample.
 * set_unfused(h, 1) sends a route-1 plan down route 0 (tests and measurement, as redio_chain_set_unfused): the same bits.
 * reserve(h, n_in) sizes route 0's scratch (the transform's staging included) for calls of up to n_in values on the plan's CURRENT
 *   route, after which an enqueue neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED
 *   while the stream is being captured).  On route 1 it does nothing.
 * enqueue: launches only, on the caller's stream; every argument is checked before anything is launched.  NULL handle or buffers,
 *   overlapping buffers (d_in == d_out included), either pointer not 8-byte aligned -> REDIO_ERR_ARG; fewer than P M values ->
 *   REDIO_OK, no launch.
 * set_chunk_rows: input rows per pass of route 0 (0 restores the 64 MiB default) -- for tests of the chunk seam; the same bits. */
typedef struct redio_pfb_synth redio_pfb_synth;
int redio_pfb_synth_create(redio_pfb_synth **h, const float *proto_taps_host, int nchan, int taps_per_branch, unsigned flags);
int redio_pfb_synth_destroy(redio_pfb_synth *h);
size_t redio_pfb_synth_nout(const redio_pfb_synth *h, size_t n_in); /* samples out for n_in cf32 values in */
int redio_pfb_synth_route(const redio_pfb_synth *h);                /* 1 the 64-channel wave kernel, 0 two passes; 0 for NULL */
int redio_pfb_synth_is_fused(const redio_pfb_synth *h);
int redio_pfb_synth_set_unfused(redio_pfb_synth *h, int unfused);
int redio_pfb_synth_set_chunk_rows(redio_pfb_synth *h, size_t rows);
int redio_pfb_synth_reserve(redio_pfb_synth *h, size_t n_in);
int redio_pfb_synth_enqueue(redio_pfb_synth *h, const void *d_rows_c32, size_t n_in, void *d_out_c32, void *stream);

/* ---- the oversampled channelizer: a row of nchan channels every hop <= nchan samples (a NEW composition) ----
 * redio_pfb_* is critically sampled: a row of M channels every M samples, so the prototype's transition band aliases back into the
 * channel edges.  This is the weighted overlap-add bank with the same prototype and transform and a hop H < M between rows (H = M / 2,
 * 2x oversampling, is the common case): every channel comes out at M / H times its bandwidth and nothing aliases into its passband.
 * M = nchan, P = taps_per_branch, H = hop with 1 <= H <= M; the prototype has M P taps in the channelizer's layout,
 * g_m[p] = proto[M p + m].  For a call on n_in cf32 samples with first_row = F:
 *     rows = (n_in - M P) / H + 1 (integer division) when n_in >= M P, else 0 (at H = M: redio_pfb_nrows);
 *     u_r[m] = the fold of dsputils::convolve (dsputils.rs:31) over x[r H + M p + m] * g_m[p], from 0.0f in ascending p = 0 .. P - 1:
 *       multiply and add rounded separately, or fmaf with REDIO_FIR_FUSED -- the bits of redio_fir on that column;
 *     v_r[(m + s_r) mod M] = u_r[m] with s_r = ((F + r) H) mod M: a permutation, no arithmetic;
 *     output row r = kissfft's forward M-point transform of v_r (the bits of a forward redio_fft); layout [row][M], natural channel
 *       order, packed.
 * With the shift channel k of every row is referred to absolute time: X_r[k] = sum_n h[n] x[r H + n] W^(k ((F + r) H + n)),
 * W = e^(-2 pi i / M), so a call on a later part of a stream continues an earlier one when F is the index of its first row.  F + rows
 * must not pass 2^64.  At H = M the shift is 0 and the rows are redio_pfb_enqueue's (ngroups = 1), bit for bit.
 * create: NULL h / taps, nchan < 1, taps_per_branch < 1 (what redio_pfb_create refuses), hop == 0 or hop > nchan -> REDIO_ERR_ARG;
 *   a size redio_fft_create refuses -> its error.  flags: REDIO_FIR_FUSED or 0, or-ed with REDIO_PFB_OS_BLOCK for route 2.
 * redio_pfb_os_route() says what a call on the plan runs (0 for NULL):
 *   1  nchan = 64, hop = 32 with taps_per_branch in {4, 8, 16} is ONE kernel, a wavefront per run of output rows (is_fused() == 1):
 *      8 bytes read and 16 written per input sample, no scratch; it captures without a reserve.
 *   2  with REDIO_PFB_OS_BLOCK in flags: nchan in {32, 128, 256, 512, 1024}, hop = nchan / 2 with taps_per_branch in {4, 8, 16} is
 *      ONE kernel, a workgroup per group of row streams (the one-kernel channelizer with a hop of half a row; is_fused() stays 0, as
 *      on redio_pfb_pspec's route 2): the same bytes, no scratch; it captures without a reserve.  Any 8-byte aligned d_in and d_out:
 *      the kernel takes 16-byte loads and stores where the pointers allow them and 8-byte ones otherwise, never route 0.  ONE
 *      shape is left out: 1024 channels x 16 taps, whose two register windows only fit with spills to scratch;
 *      it stays on route 0.  On every other shape the flag is accepted and changes nothing (64 channels at hop 32 stay route 1).
 *   0  every other plan runs a branch pass (row stride H, rotated store) into plan-owned scratch and its own forward redio_fft over
 *      those rows, in chunks of at most 64 MiB of whole rows.
 * set_unfused(h, 1) sends a route-1 or route-2 plan down route 0 (tests and measurement, as redio_chain_set_unfused), set_unfused(h, 0)
 *   brings it back: the same bits.
 * reserve(h, n_in) sizes route 0's scratch (the transform's staging included) for calls of up to n_in samples on the plan's CURRENT
 *   route, after which an enqueue neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED
 *   while the stream is being captured).  On routes 1 and 2 it does nothing.
 * enqueue: launches only, on the caller's stream; every argument is checked before anything is launched.  NULL handle or buffers,
 *   overlapping buffers (d_in == d_out included), either pointer not 8-byte aligned -> REDIO_ERR_ARG; fewer than M P samples ->
 *   REDIO_OK, no launch.  Samples behind the last row's window are not read.
 * set_chunk_rows: rows per pass of route 0 (0 restores the 64 MiB default) -- for tests of the chunk seam; the same bits. */
#define REDIO_PFB_OS_BLOCK 4u /* redio_pfb_os_create flags: the workgroup kernel (route 2) where the shape has one */
typedef struct redio_pfb_os redio_pfb_os;
int redio_pfb_os_create(redio_pfb_os **h, const float *proto_taps_host, int nchan, int taps_per_branch, size_t hop, unsigned flags);
int redio_pfb_os_destroy(redio_pfb_os *h);
size_t redio_pfb_os_nrows(const redio_pfb_os *h, size_t n_in); /* rows of nchan cf32 out for n_in cf32 samples in */
size_t redio_pfb_os_hop(const redio_pfb_os *h);                /* 0 for NULL */
int redio_pfb_os_route(const redio_pfb_os *h);                 /* 1 the 64-channel wave kernel, 2 the workgroup kernel, 0 two passes; 0 for NULL */
int redio_pfb_os_is_fused(const redio_pfb_os *h);
int redio_pfb_os_set_unfused(redio_pfb_os *h, int unfused);
int redio_pfb_os_set_chunk_rows(redio_pfb_os *h, size_t rows);
int redio_pfb_os_reserve(redio_pfb_os *h, size_t n_in);
int redio_pfb_os_enqueue(redio_pfb_os *h, const void *d_in_c32, size_t n_in, uint64_t first_row, void *d_out_c32, void *stream);

/* ---- the channelizer's one exchange step over RCCL / xGMI (the only collective on the path) ----
 * Time-sharded channelizer: every rank runs redio_pfb_enqueue(..., ngroups = G) on its own slice of the stream and
 * holds d_grouped = [G groups][its rows][chans_per_rank cf32]; the exchange sends group q to rank q
 * (ncclGroupStart; ncclSend/ncclRecv per peer; ncclGroupEnd), so that afterwards rank g holds
 * d_out = [sum(rows_per_rank) rows, in rank (= time) order][chans_per_rank cf32] for ITS channels.
 * rows_per_rank[G] (host) may be ragged.  Enqueued on `stream`; nothing synchronises.
 * librccl.so is loaded on first use; REDIO_ERR_COMM (text: redio_comm_last_error) if it is missing or a call fails.
 * One rank per process: rank 0 calls redio_comm_unique_id, the launcher hands the 128 bytes to every rank, every rank
 * calls redio_comm_init_rank on its own device.  Several ranks in one process (the reference's thread-per-block host):
 * redio_comm_init_all(comms, ndev, devices) then redio_pfb_exchange_all, which wraps all ranks' transfers in one group.
 * Test seam: when the environment variable REDIO_RCCL_LIB is set, the library at that path is the transport (loaded with
 * RTLD_LOCAL on first use, its nine nccl* entry points resolved from it) and nothing else is tried; if it cannot be loaded or
 * lacks an entry point every redio_comm_* call returns REDIO_ERR_COMM and redio_comm_last_error names the path.  The tests use
 * it to run the exchange with several ranks on one device (tests/stub/fake_rccl.cpp); it is never set by the library or the host layer. */
#define REDIO_COMM_ID_BYTES 128
typedef struct redio_comm redio_comm;
int redio_comm_unique_id(void *id128);
int redio_comm_init_rank(redio_comm **c, int nranks, int rank, const void *id128);
int redio_comm_init_all(redio_comm **comms, int ndev, const int *devices /* NULL = 0..ndev-1 */);
int redio_comm_destroy(redio_comm *c);
int redio_comm_rank(const redio_comm *c);
int redio_comm_size(const redio_comm *c);
const char *redio_comm_last_error(void); /* text of the calling thread's last REDIO_ERR_COMM */
int redio_pfb_exchange(redio_comm *c, const void *d_grouped, void *d_out, const size_t *rows_per_rank, size_t chans_per_rank, void *stream);
/* the same with rank q's rows placed at row out_row_offset[q] of d_out: lets a slice be analysed in pieces whose exchanges run beside
 * the analysis of the next piece on another HIP stream and still build the time-ordered result in place */
int redio_pfb_exchange_at(redio_comm *c, const void *d_grouped, void *d_out, const size_t *rows_per_rank, const size_t *out_row_offset,
                          size_t chans_per_rank, void *stream);
int redio_pfb_exchange_all(redio_comm *const *comms, int ndev, const void *const *d_grouped, void *const *d_out,
                           const size_t *rows_per_rank, size_t chans_per_rank, void *const *streams);

/* ---- carried history: the windowed plans above as STREAMS (BASELINE.json configs[1] "history carried") ----
 * redio_fir_enqueue & co. are stateless per call, like dsputils::convolve (dsputils.rs:30-32), which loses ntaps-1
 * outputs at every message seam.  A *_stream handle sits on a plan (not owned: destroy the stream first) and keeps the
 * stream's unconsumed tail (fewer samples than one window) on the device, so that feeding a stream in ANY pieces gives
 * exactly the bits of one stateless call on the whole stream:
 *     fir:    y[i] = fold_j x[decim*i + j]*taps[j] for every i whose window has arrived (decimation phase 0 at stream start)
 *     chain:  spectrum b from decimated samples [b*nfft, (b+1)*nfft) of that y
 *     pfb:    row t from input rows t .. t+taps_per_branch-1 (layout [row][nchan] only)
 *     ovsave: block b -> hop outputs, blocks every hop samples from the stream start (ovsave_real: the same on f32 samples; d_new
 *             needs 4-byte alignment only -- messages may have any length, odd ones included -- and d_out 8-byte alignment)
 *     pspec:  row r from the W = (integrate - 1) step + nfft samples that start at r * integrate * step; *nout counts f32 words
 *             (whole rows of nfft).  The staging buffers hold fewer than W samples each side of a seam -- 8 MiB of history at
 *             nfft = integrate = 1024 -- so a long integration costs that much device memory per stream handle.  (A u8 stream,
 *             redio_pspec_stream_create_u8, carries the same samples as bytes: a quarter of that.)
 *     pspec_real: the same on f32 samples (W and H count real samples), rows of nfft / 2 + 1 f32; d_new needs 4-byte alignment only --
 *             messages may have any length, odd ones included -- and so does d_out.  Create reserves for the seam windows
 *             (redio_pspec_real_reserve(plan, largest message + W) keeps longer bodies allocation-free).
 * enqueue() writes *nout (= redio_*_stream_nout(h, n_new), known before the call) output samples to d_out; the new
 * samples are read in place (only a seam of fewer than one window is staged through a plan-owned buffer).  It only
 * launches kernels and small device copies -- with one exception: a plan shape that runs as two kernels (redio_chain_is_fused() == 0,
 * or a body that starts on an odd sample) keeps a plan-owned intermediate that *_stream_create sizes for the seam windows and
 * that grows on a longer body: call redio_chain_reserve(plan, largest message) once to keep enqueue allocation-free.
 * The host-side counters advance only when every kernel of the call has been launched (a failed call can be repeated); feed one
 * stream from one thread in order -- a call that finds another thread inside enqueue() / reset() of the same handle returns
 * REDIO_ERR_ARG.  Not graph-capturable (the split changes from call to call).  pending() = samples carried. */
typedef struct redio_fir_stream redio_fir_stream;
int redio_fir_stream_create(redio_fir_stream **h, redio_fir *plan);
int redio_fir_stream_destroy(redio_fir_stream *h);
int redio_fir_stream_reset(redio_fir_stream *h);
size_t redio_fir_stream_nout(const redio_fir_stream *h, size_t n_new);
size_t redio_fir_stream_pending(const redio_fir_stream *h);
int redio_fir_stream_enqueue(redio_fir_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
typedef struct redio_chain_stream redio_chain_stream;
int redio_chain_stream_create(redio_chain_stream **h, redio_chain *plan);
int redio_chain_stream_destroy(redio_chain_stream *h);
int redio_chain_stream_reset(redio_chain_stream *h);
size_t redio_chain_stream_nout(const redio_chain_stream *h, size_t n_new);
size_t redio_chain_stream_pending(const redio_chain_stream *h);
int redio_chain_stream_enqueue(redio_chain_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
typedef struct redio_pfb_stream redio_pfb_stream;
int redio_pfb_stream_create(redio_pfb_stream **h, redio_pfb *plan);
/* the chain / channelizer streams fed with the receiver's interleaved u8 I/Q bytes (rtlsdr.rs:127-162): d_new points to bytes,
 * n_new still counts SAMPLES (2 bytes each); the history is carried as bytes and every window runs redio_*_enqueue_u8.
 * All other redio_{chain,pfb}_stream_* calls apply unchanged. */
int redio_chain_stream_create_u8(redio_chain_stream **h, redio_chain *plan);
int redio_pfb_stream_create_u8(redio_pfb_stream **h, redio_pfb *plan);
int redio_pfb_stream_destroy(redio_pfb_stream *h);
int redio_pfb_stream_reset(redio_pfb_stream *h);
size_t redio_pfb_stream_nout(const redio_pfb_stream *h, size_t n_new);
size_t redio_pfb_stream_pending(const redio_pfb_stream *h);
int redio_pfb_stream_enqueue(redio_pfb_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
typedef struct redio_ovsave_stream redio_ovsave_stream;
int redio_ovsave_stream_create(redio_ovsave_stream **h, redio_ovsave *plan);
int redio_ovsave_stream_destroy(redio_ovsave_stream *h);
int redio_ovsave_stream_reset(redio_ovsave_stream *h);
size_t redio_ovsave_stream_nout(const redio_ovsave_stream *h, size_t n_new);
size_t redio_ovsave_stream_pending(const redio_ovsave_stream *h);
int redio_ovsave_stream_enqueue(redio_ovsave_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
typedef struct redio_ovsave_real_stream redio_ovsave_real_stream;
int redio_ovsave_real_stream_create(redio_ovsave_real_stream **h, redio_ovsave_real *plan);
int redio_ovsave_real_stream_destroy(redio_ovsave_real_stream *h);
int redio_ovsave_real_stream_reset(redio_ovsave_real_stream *h);
size_t redio_ovsave_real_stream_nout(const redio_ovsave_real_stream *h, size_t n_new);
size_t redio_ovsave_real_stream_pending(const redio_ovsave_real_stream *h);
int redio_ovsave_real_stream_enqueue(redio_ovsave_real_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
typedef struct redio_pspec_stream redio_pspec_stream;
int redio_pspec_stream_create(redio_pspec_stream **h, redio_pspec *plan);
int redio_pspec_stream_destroy(redio_pspec_stream *h);
int redio_pspec_stream_reset(redio_pspec_stream *h);
size_t redio_pspec_stream_nout(const redio_pspec_stream *h, size_t n_new);
size_t redio_pspec_stream_pending(const redio_pspec_stream *h);
int redio_pspec_stream_enqueue(redio_pspec_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
/* the power-spectrum stream fed with the receiver's interleaved u8 I/Q bytes, as the chain / channelizer ones above: d_new points to
 * bytes (2-byte aligned: an odd address is REDIO_ERR_ARG before anything is launched), n_new still counts SAMPLES; the history is carried as bytes and every window runs redio_pspec_enqueue_u8.
 * Create reserves for the seam windows (redio_pspec_reserve_u8(plan, largest message's bytes + 2 W) keeps longer bodies allocation-free).
 * All other redio_pspec_stream_* calls apply unchanged. */
int redio_pspec_stream_create_u8(redio_pspec_stream **h, redio_pspec *plan);
typedef struct redio_pspec_real_stream redio_pspec_real_stream;
int redio_pspec_real_stream_create(redio_pspec_real_stream **h, redio_pspec_real *plan);
int redio_pspec_real_stream_destroy(redio_pspec_real_stream *h);
int redio_pspec_real_stream_reset(redio_pspec_real_stream *h);
size_t redio_pspec_real_stream_nout(const redio_pspec_real_stream *h, size_t n_new);
size_t redio_pspec_real_stream_pending(const redio_pspec_real_stream *h);
int redio_pspec_real_stream_enqueue(redio_pspec_real_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
/* the polyphase spectrometer as a stream: row r from the W = (integrate - 1 + taps_per_branch) nchan samples that start at
 * r * integrate * nchan; *nout counts f32 words (whole rows of nchan).  create_u8: d_new points to interleaved u8 I/Q bytes (2-byte
 * aligned: an odd address is REDIO_ERR_ARG before anything is launched), n_new still counts SAMPLES, the history is carried as bytes.
 * Create reserves for the seam windows (redio_pfb_pspec_reserve / _reserve_u8 for the largest message + W keeps longer bodies
 * allocation-free on the shapes that are not fused). */
typedef struct redio_pfb_pspec_stream redio_pfb_pspec_stream;
int redio_pfb_pspec_stream_create(redio_pfb_pspec_stream **h, redio_pfb_pspec *plan);
int redio_pfb_pspec_stream_create_u8(redio_pfb_pspec_stream **h, redio_pfb_pspec *plan);
int redio_pfb_pspec_stream_destroy(redio_pfb_pspec_stream *h);
int redio_pfb_pspec_stream_reset(redio_pfb_pspec_stream *h);
size_t redio_pfb_pspec_stream_nout(const redio_pfb_pspec_stream *h, size_t n_new);
size_t redio_pfb_pspec_stream_pending(const redio_pfb_pspec_stream *h);
int redio_pfb_pspec_stream_enqueue(redio_pfb_pspec_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
/* the tuner as a stream (kpn.rs:198-203, dsputils.rs:30-32): carried history AND carried phase -- the handle passes the stream index of
 * every window's first sample to the plan as first_index, so any segmentation gives the bits of one redio_ddc_enqueue on the whole
 * stream with first_index 0.  create_u8: d_new points to interleaved u8 I/Q bytes (any alignment), n_new still counts SAMPLES.
 * redio_ddc_stream_index: the stream index of the next new sample (0 after create and reset; unchanged by a failed call). */
typedef struct redio_ddc_stream redio_ddc_stream;
int redio_ddc_stream_create(redio_ddc_stream **h, redio_ddc *plan);
int redio_ddc_stream_create_u8(redio_ddc_stream **h, redio_ddc *plan);
int redio_ddc_stream_destroy(redio_ddc_stream *h);
int redio_ddc_stream_reset(redio_ddc_stream *h);
size_t redio_ddc_stream_nout(const redio_ddc_stream *h, size_t n_new);
size_t redio_ddc_stream_pending(const redio_ddc_stream *h);
int redio_ddc_stream_enqueue(redio_ddc_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
uint64_t redio_ddc_stream_index(const redio_ddc_stream *h);
/* the rational resampler as a stream (dsputils.rs:30-32, redio_upfirdn_*'s contract): the unit is one PERIOD -- U' outputs from the Wp
 * samples that start at a multiple of D' samples of the stream, which is phase 0, so samples are carried and no phase.  The stream emits
 * whole periods: after N samples in any pieces it has written the first U' * max(0, (N - Wp) / D' + 1) outputs of one
 * redio_upfirdn_enqueue on the whole stream, bit for bit (that call may end with a few more outputs, which only the stateless call
 * gives).  *nout and _stream_nout count samples. */
typedef struct redio_upfirdn_stream redio_upfirdn_stream;
int redio_upfirdn_stream_create(redio_upfirdn_stream **h, redio_upfirdn *plan);
int redio_upfirdn_stream_destroy(redio_upfirdn_stream *h);
int redio_upfirdn_stream_reset(redio_upfirdn_stream *h);
size_t redio_upfirdn_stream_nout(const redio_upfirdn_stream *h, size_t n_new);
size_t redio_upfirdn_stream_pending(const redio_upfirdn_stream *h);
int redio_upfirdn_stream_enqueue(redio_upfirdn_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
/* the tuned resampler as a stream (kpn.rs:198-203, dsputils.rs:30-32): the resampler's geometry and the tuner's phase.  The unit is one
 * PERIOD -- U' outputs from the Wp samples that start at a multiple of D' samples of the stream -- and the handle passes the stream index
 * of every window's first sample to the plan as first_index.  After N samples in any pieces the stream has written the first
 * U' * max(0, (N - Wp) / D' + 1) outputs of one redio_ddc_upfirdn_enqueue on the whole stream with first_index 0, bit for bit.
 * create_u8: d_new points to interleaved u8 I/Q bytes (any alignment), carried as bytes; n_new still counts SAMPLES.  *nout and
 * _stream_nout count output samples.  _stream_index: the stream index of the next new sample (0 after create and reset; unchanged by a
 * failed call). */
typedef struct redio_ddc_upfirdn_stream redio_ddc_upfirdn_stream;
int redio_ddc_upfirdn_stream_create(redio_ddc_upfirdn_stream **h, redio_ddc_upfirdn *plan);
int redio_ddc_upfirdn_stream_create_u8(redio_ddc_upfirdn_stream **h, redio_ddc_upfirdn *plan);
int redio_ddc_upfirdn_stream_destroy(redio_ddc_upfirdn_stream *h);
int redio_ddc_upfirdn_stream_reset(redio_ddc_upfirdn_stream *h);
size_t redio_ddc_upfirdn_stream_nout(const redio_ddc_upfirdn_stream *h, size_t n_new);
size_t redio_ddc_upfirdn_stream_pending(const redio_ddc_upfirdn_stream *h);
int redio_ddc_upfirdn_stream_enqueue(redio_ddc_upfirdn_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
uint64_t redio_ddc_upfirdn_stream_index(const redio_ddc_upfirdn_stream *h);
/* the synthesis filterbank as a stream: the unit is one output row (nchan samples) from the P nchan values that start at a multiple of
 * nchan values of the stream, so P - 1 whole rows and the values of a partial row are carried.  A message may have any length (d_new
 * 8-byte aligned); whole output rows are emitted, and a stream fed in any pieces concatenates to one redio_pfb_synth_enqueue on the
 * whole stream, bit for bit.  Create reserves the plan's scratch for the seam windows (redio_pfb_synth_reserve for the largest
 * message + P nchan keeps longer bodies allocation-free on route 0).  *nout and _stream_nout count samples; pending() = values carried. */
typedef struct redio_pfb_synth_stream redio_pfb_synth_stream;
int redio_pfb_synth_stream_create(redio_pfb_synth_stream **h, redio_pfb_synth *plan);
int redio_pfb_synth_stream_destroy(redio_pfb_synth_stream *h);
int redio_pfb_synth_stream_reset(redio_pfb_synth_stream *h);
size_t redio_pfb_synth_stream_nout(const redio_pfb_synth_stream *h, size_t n_new);
size_t redio_pfb_synth_stream_pending(const redio_pfb_synth_stream *h);
int redio_pfb_synth_stream_enqueue(redio_pfb_synth_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);
/* the oversampled channelizer as a stream, on the conventions of redio_pfb_stream_*: the unit is one row (nchan cf32) from the
 * P nchan samples that start at a multiple of hop samples of the stream.  The handle carries the unconsumed samples -- everything from
 * the next row's first sample on -- and the running row index, which is every call's first_row: the shift continues across messages.
 * A message may have any length (d_new 8-byte aligned); a stream fed in any pieces concatenates to one redio_pfb_os_enqueue with
 * first_row = 0 on the whole stream, bit for bit.  reset zeroes both.  Create reserves the plan's scratch for the seam windows
 * (redio_pfb_os_reserve for the largest message + P nchan keeps longer bodies allocation-free on route 0).  *nout and _stream_nout
 * count output SAMPLES (rows * nchan); pending() = samples carried. */
typedef struct redio_pfb_os_stream redio_pfb_os_stream;
int redio_pfb_os_stream_create(redio_pfb_os_stream **h, redio_pfb_os *plan);
int redio_pfb_os_stream_destroy(redio_pfb_os_stream *h);
int redio_pfb_os_stream_reset(redio_pfb_os_stream *h);
size_t redio_pfb_os_stream_nout(const redio_pfb_os_stream *h, size_t n_new);
size_t redio_pfb_os_stream_pending(const redio_pfb_os_stream *h);
int redio_pfb_os_stream_enqueue(redio_pfb_os_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);

/* ---- A6: samplerate::resample's native side, src/samplerate/src/samplerate.rs:59-87 ----
 * nchan independent mono streams that share ratio and block lengths (the reference creates one
 * src_new(SRC_SINC_MEDIUM_QUALITY, 1) state per block, :61).  Control flow, output count law and
 * arithmetic order are those of the published libsamplerate 0.1.8 sinc converter; the coefficient
 * table is a stated design.  Bit-identical to oracle/oracle_src.c.
 * Return values: REDIO_OK, a negative redio error, or one of the library's positive error codes. */
enum {
    REDIO_SRC_ERR_MALLOC_FAILED = 1, REDIO_SRC_ERR_BAD_STATE = 2, REDIO_SRC_ERR_BAD_DATA = 3,
    REDIO_SRC_ERR_BAD_DATA_PTR = 4, REDIO_SRC_ERR_NO_PRIVATE = 5, REDIO_SRC_ERR_BAD_SRC_RATIO = 6,
    REDIO_SRC_ERR_BAD_PROC_PTR = 7, REDIO_SRC_ERR_SHIFT_BITS = 8, REDIO_SRC_ERR_FILTER_LEN = 9,
    REDIO_SRC_ERR_BAD_CONVERTER = 10, REDIO_SRC_ERR_BAD_CHANNEL_COUNT = 11,
    REDIO_SRC_ERR_SINC_BAD_BUFFER_LEN = 12, REDIO_SRC_ERR_SIZE_INCOMPATIBILITY = 13,
    REDIO_SRC_ERR_BAD_PRIV_PTR = 14, REDIO_SRC_ERR_BAD_SINC_STATE = 15, REDIO_SRC_ERR_DATA_OVERLAP = 16,
    REDIO_SRC_ERR_BAD_CALLBACK = 17, REDIO_SRC_ERR_BAD_MODE = 18, REDIO_SRC_ERR_NULL_CALLBACK = 19,
    REDIO_SRC_ERR_NO_VARIABLE_RATIO = 20, REDIO_SRC_ERR_SINC_PREPARE_DATA_BAD_LEN = 21,
    REDIO_SRC_ERR_BAD_INTERNAL_STATE = 22
};
typedef struct redio_src redio_src;
/* converter (samplerate.rs:26-30): 0 best / 1 medium / 2 fastest sinc, 3 zero-order hold, 4 linear; anything else
 * REDIO_SRC_ERR_BAD_CONVERTER (the reference only ever asks for 1).  nchan independent mono streams, stored as rows. */
int redio_src_create(redio_src **h, int converter, int nchan);
int redio_src_destroy(redio_src *h);
int redio_src_reset(redio_src *h);
int redio_src_set_ratio(redio_src *h, double ratio);
/* arithmetic of the device-resident form.  EXACT (default): double accumulation in the library's
 * order, bit-identical to the oracle; calls whose phase is uniform (constant ratio, 1/ratio an
 * integer, no end_of_input) run as one launch.  FAST: those uniform calls use an f32 polyphase
 * filter bank (taps rounded to f32, f32 accumulation) - NOT bit-identical, error bounded by
 * ntaps * 2^-23 * sum|h| * max|x|; every other call still runs EXACT.  EPOCHS: EXACT with one
 * launch per buffer refill, the literal schedule of the library (kept for cross-checks). */
enum { REDIO_SRC_EXACT = 0, REDIO_SRC_FAST = 1, REDIO_SRC_EPOCHS = 2 };
int redio_src_set_mode(redio_src *h, int mode);
/* device-resident: d_in[nchan][in_stride], d_out[nchan][out_stride] f32; synchronises the stream
 * before returning (per-output parameters are produced by the host state machine) */
int redio_src_process(redio_src *h, const void *d_in, long input_frames, long in_stride, void *d_out, long output_frames,
                      long out_stride, double src_ratio, int end_of_input, long *input_frames_used,
                      long *output_frames_gen, void *stream);
/* redio_src_process(..., end_of_input = 0, ...) in stream order: the same outputs, counts, error codes and carried state for every
 * converter, ratio and mode, and the two entries (with reset / set_ratio / set_mode) may be mixed freely on one handle.
 *   QUEUED: a call the single-launch uniform path serves (constant ratio, 1/ratio an integer <= 256, sinc converters, EXACT or FAST)
 *   whose tables for that increment already exist only launches kernels on `stream`: no synchronisation, no copy, no allocation; the
 *   counts are final when the call returns.  d_in must stay valid until the stream has passed the call.
 *   SYNCHRONISED: every other call (the first at a new increment, a varying or non-integer 1/ratio, a ratio that fell below the
 *   history kept, converters 3 / 4, a shape without a single-launch kernel) runs redio_src_process's path including its wait.
 * out_stride == 0: packed rows, d_out[nchan][*output_frames_gen]; nothing behind nchan * gen floats is written (d_out holds
 * nchan * output_frames floats at most).  One handle belongs to one stream at a time; the caller orders its use on different streams.
 * Not capturable (see redio_graph_begin): REDIO_ERR_UNSUPPORTED on a capturing stream, state untouched. */
int redio_src_enqueue(redio_src *h, const void *d_in, long input_frames, long in_stride, void *d_out, long output_frames,
                      long out_stride, double src_ratio, long *input_frames_used, long *output_frames_gen, void *stream);
/* calls of redio_src_enqueue on this handle that were queued / that synchronised */
int redio_src_enqueue_counts(const redio_src *h, long *queued, long *synchronised);
/* host buffers, interleaved frames of the handle's nchan channels (mono: plain samples), synchronous: the body of the
 * src_process drop-in (include/samplerate.h); every channel is converted exactly as a mono stream */
int redio_src_process_host(redio_src *h, const float *data_in, long input_frames, float *data_out, long output_frames,
                           double src_ratio, int end_of_input, long *input_frames_used, long *output_frames_gen);
/* diagnostics: buffer-refill epochs of this handle served by the periodic-phase kernel (constant rational ratios such as
 * 48000/44100 or 2.0: P sets of coefficients, LDS tiles) and by the general per-tap kernel; both bit-identical */
int redio_src_path_counts(const redio_src *h, long *periodic, long *general);
/* the coefficient table of a converter (coeffs_out may be NULL; it holds half_len + 2 floats) */
int redio_src_table(int converter, float *coeffs_out, int *half_len, int *increment);

/* ---- kpn vector maps on device: mul_vecs (src/kpn/src/kpn.rs:198-203) and sum_vecs (:227-231) ----
 * out[i] = a[i] * b[i] / a[i] + b[i] for i < n (the caller passes n = min of the two lengths, as zip does);
 * f32 and Complex<f32> ((ar*br - ai*bi, ar*bi + ai*br), every operation rounded on its own). */
int redio_mul_f32(const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int redio_add_f32(const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int redio_mul_c32(const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);
int redio_add_c32(const void *d_a, const void *d_b, void *d_out, size_t n, void *stream);

/* ---- layout: the channelizer's rows <-> one contiguous mono stream per channel component ----
 * d_rows cf32 [nrows][nchan] (redio_pfb_enqueue's output); d_planes f32 [2*nchan][plane_stride]: plane 2c = Re of channel c, plane
 * 2c + 1 = Im, each plane uses its first nrows entries (the rest is not touched) -- redio_src_enqueue's rows for 2*nchan channels.
 * Pure data movement: every 32-bit word arrives unchanged.  nrows == 0: REDIO_OK, no launch; nchan < 1, plane_stride < nrows, or a
 * NULL / not 4-byte aligned pointer with work to do: REDIO_ERR_ARG.  Launch only (capturable). */
int redio_rows_to_planes_c32(const void *d_rows, size_t nrows, int nchan, void *d_planes, size_t plane_stride, void *stream);
int redio_planes_to_rows_c32(const void *d_planes, size_t plane_stride, size_t nrows, int nchan, void *d_rows, void *stream);

/* order-free 64-bit sum of the n 32-bit words at d_words, ADDED to the u64 at d_sum_u64 (device memory the caller zeroed; one atomic
 * per workgroup): the checking sink of a device-resident graph -- reads every word a block produced, exact whatever the order */
int redio_checksum_u32(const void *d_words, size_t n, void *d_sum_u64, void *stream);

/* ---- synthetic input: hash-generated cf32 / f32 in [-1, 1), device side ---- */
int redio_synth_iq(void *d_out, uint32_t seed, uint64_t first_sample, size_t n, void *stream);
int redio_synth_f32(void *d_out, uint32_t seed, uint64_t first_sample, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
/* the oversampled synthesis bank, the way back from the oversampled channelizer's rows to one stream: its contract
 * and declarations, in the style of the plans above, are in a header of their own that this one brings in */
#include "redio_pfb_os_synth.h"
#endif /* REDIO_H */
