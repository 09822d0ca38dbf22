/* redio_pfb_os_synth.h -- the oversampled synthesis bank of the C ABI (redio.h includes this header; the error codes, REDIO_FIR_FUSED and
 * the conventions of every plan are stated there). */
#ifndef REDIO_PFB_OS_SYNTH_H
#define REDIO_PFB_OS_SYNTH_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---- the oversampled synthesis bank: redio_pfb_os_*'s rows back into one stream (a NEW composition) ----
 * redio_pfb_synth_* takes rows that are M samples apart.  This is the other half of the weighted overlap-add pair: rows that are
 * H <= M samples apart, as redio_pfb_os_enqueue writes them, are transformed back and overlap-added into one stream.
 * M = nchan, P = taps_per_branch, H = hop with 1 <= H <= M; the prototype h has M P taps in the channelizer's layout;
 * L = ceil(P M / H).  The input is T = n_in / M (integer division) rows X_r[0 .. M) of cf32 in natural channel order; a trailing
 * partial row is ignored.  first_row = F is the index of the call's first row on the analysis side; F + T must not pass 2^64.
 *     w_r = kissfft's unnormalised M-point inverse transform of X_r (the bits of an inverse redio_fft);
 *     n_out = (T - L + 1) H samples when T >= L, else 0;
 *     output sample n = q H + j (0 <= j < H) lies at absolute time tau = (F + L - 1) H + n;
 *     y[n] = the strict left fold of dsputils::convolve (dsputils.rs:31) from 0.0f, in ascending row r = q .. q + L - 1, over the rows
 *       whose window offset o = tau - (F + r) H satisfies 0 <= o < P M (every row when H divides P M; otherwise the oldest row drops
 *       out for the residues j with (L - 1) H + j >= P M), of w_r[tau mod M] * h[tap(o)], tap(o) = (P - 1 - o div M) M + o mod M:
 *       multiply and add rounded separately, or fmaf with REDIO_FIR_FUSED.  There is no 1 / M.
 * At H = M this is redio_pfb_synth_enqueue term for term, for every F: the two are bit-equal.  A prototype prepared for
 * redio_pfb_synth keeps its meaning at every hop (each M-branch's p order flipped: h[tap(o)] = g[o] for a synthesis window g).  With
 * an analysis window a and a synthesis window g on window positions [0, M) and sum_r a[i - r H] g[i - r H] = 1,
 * os_synth(pfb_os(x, F), F)[n] = M x[(L - 1) H + n] up to the transforms' rounding, for any F used on both sides.
 * create: NULL h / taps, nchan < 1, taps_per_branch < 1, hop == 0 or hop > nchan -> REDIO_ERR_ARG; a size redio_fft_create refuses ->
 *   its error.  flags: REDIO_FIR_FUSED or 0.
 * redio_pfb_os_synth_route() says what a call on the plan runs (0 for NULL):
 *   1  nchan = 64, hop = 32 with taps_per_branch in {4, 8, 16} is ONE kernel, a wavefront per run of output hops (is_fused() == 1):
 *      8 bytes read and 4 written per channel value, no scratch; it captures without a reserve.
 *   0  every other plan runs its own inverse redio_fft over the rows into plan-owned scratch and an overlap-add pass, in chunks of at
 *      most 64 MiB of whole rows that overlap by L - 1 rows.
 * set_unfused(h, 1) sends a route-1 plan down route 0 (tests and measurement, as redio_chain_set_unfused): the same bits.
 * reserve(h, n_in) sizes route 0's scratch (the transform's staging included) for calls of up to n_in values on the plan's CURRENT
 *   route, after which an enqueue neither allocates nor synchronises; un-reserved it grows on first use (REDIO_ERR_NOT_RESERVED
 *   while the stream is being captured).  On route 1 it does nothing.
 * enqueue: launches only, on the caller's stream; every argument is checked before anything is launched.  NULL handle or buffers,
 *   overlapping buffers (d_rows == d_out included), either pointer not 8-byte aligned -> REDIO_ERR_ARG; fewer than L rows ->
 *   REDIO_OK, no launch.
 * set_chunk_rows: input rows per pass of route 0 (0 restores the 64 MiB default; fewer than L count as L) -- for tests of the chunk
 *   seam; the same bits. */
typedef struct redio_pfb_os_synth redio_pfb_os_synth;
int redio_pfb_os_synth_create(redio_pfb_os_synth **h, const float *proto_taps_host, int nchan, int taps_per_branch, size_t hop, unsigned flags);
int redio_pfb_os_synth_destroy(redio_pfb_os_synth *h);
size_t redio_pfb_os_synth_nout(const redio_pfb_os_synth *h, size_t n_in); /* cf32 samples out for n_in cf32 channel values in */
size_t redio_pfb_os_synth_hop(const redio_pfb_os_synth *h);               /* 0 for NULL */
int redio_pfb_os_synth_route(const redio_pfb_os_synth *h);                /* 1 the 64-channel wave kernel, 0 two passes; 0 for NULL */
int redio_pfb_os_synth_is_fused(const redio_pfb_os_synth *h);
int redio_pfb_os_synth_set_unfused(redio_pfb_os_synth *h, int unfused);
int redio_pfb_os_synth_set_chunk_rows(redio_pfb_os_synth *h, size_t rows);
int redio_pfb_os_synth_reserve(redio_pfb_os_synth *h, size_t n_in);
int redio_pfb_os_synth_enqueue(redio_pfb_os_synth *h, const void *d_rows_c32, size_t n_in, uint64_t first_row, void *d_out_c32, void *stream);

/* the oversampled synthesis bank as a stream, on the conventions of redio_pfb_synth_stream_*: the input is channel VALUES (rows of
 * nchan cf32), the unit is one hop of `hop` output samples from the L = ceil(P nchan / hop) rows that start at a whole row of the
 * stream.  The handle carries L - 1 whole rows, the values of a partial row, and the running row index, which is every call's
 * first_row.  A message may have any length (d_new 8-byte aligned); a stream fed in any pieces concatenates to one
 * redio_pfb_os_synth_enqueue with first_row = 0 on the whole stream, bit for bit.  reset zeroes all of it.  Create reserves the plan's
 * scratch for the seam windows (redio_pfb_os_synth_reserve for the largest message + L nchan keeps longer bodies allocation-free on
 * route 0).  *nout and _stream_nout count output SAMPLES; pending() = values carried. */
typedef struct redio_pfb_os_synth_stream redio_pfb_os_synth_stream;
int redio_pfb_os_synth_stream_create(redio_pfb_os_synth_stream **h, redio_pfb_os_synth *plan);
int redio_pfb_os_synth_stream_destroy(redio_pfb_os_synth_stream *h);
int redio_pfb_os_synth_stream_reset(redio_pfb_os_synth_stream *h);
size_t redio_pfb_os_synth_stream_nout(const redio_pfb_os_synth_stream *h, size_t n_new);
size_t redio_pfb_os_synth_stream_pending(const redio_pfb_os_synth_stream *h);
int redio_pfb_os_synth_stream_enqueue(redio_pfb_os_synth_stream *h, const void *d_new, size_t n_new, void *d_out, size_t *nout, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* REDIO_PFB_OS_SYNTH_H */
