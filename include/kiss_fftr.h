/*
 * kiss_fftr.h -- drop-in for the real-input half of the kissfft library (tools/kiss_fftr.h of kissfft 1.3.0):
 *     kiss_fftr_alloc / kiss_fftr / kiss_fftri / kiss_fftr_free
 * Exported by libkissfft.so in this repo next to the kiss_fft_* symbols (kiss_fft.h); the transform runs on the MI355X through
 * redio_fftr_* (include/redio.h).  Host pageable buffers in and out, synchronous: the result is in the output when the call returns.
 *
 * nfft counts REAL points and must be even.  kiss_fftr reads nfft scalars and writes nfft/2 + 1 bins; kiss_fftri reads nfft/2 + 1
 * bins and writes nfft scalars, unnormalised (kiss_fftri(kiss_fftr(x)) = nfft * x).
 *
 * Deviations, in the manner of kiss_fft.h: the published code calls exit(1) when a transform is called on a cfg of the wrong
 * direction; here the output is filled with NaN and one line goes to stderr, as on a HIP failure.  Nothing aborts.
 */
#ifndef KISS_FFTR_H
#define KISS_FFTR_H
#include "kiss_fft.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef float kiss_fft_scalar;
typedef struct kiss_fftr_state *kiss_fftr_cfg;

/* mem/lenmem placement protocol as kiss_fft_alloc.  Odd nfft: NULL and "Real FFT optimization must be even." on stderr. */
kiss_fftr_cfg kiss_fftr_alloc(int nfft, int inverse_fft, void *mem, size_t *lenmem);
/* timedata: nfft scalars; freqdata: nfft/2 + 1 bins */
void kiss_fftr(kiss_fftr_cfg cfg, const kiss_fft_scalar *timedata, kiss_fft_cpx *freqdata);
void kiss_fftri(kiss_fftr_cfg cfg, const kiss_fft_cpx *freqdata, kiss_fft_scalar *timedata);
void kiss_fftr_free(kiss_fftr_cfg cfg); /* releases the device plan (the published macro is free()) */

#ifdef __cplusplus
}
#endif
#endif
