"""kiss_fftr / kiss_fftri (kissfft 1.3.0 tools/kiss_fftr.c, as restated in DESIGN.md) in numpy float32 over oracle.fft: the checker of the
real-input transform.  Every multiply and add is one float32 operation; the two writes of a loop step happen in loop order, so the
second one wins at k = M / 2."""
import math

import numpy as np

import oracle as O

PI = 3.141592653589793238462643383279502884197169399375105820974944  # oracle/oracle_kiss.c:61
F = np.float32
HALF = F(0.5)


def super_tw(M, inverse=False):
    ph = [-PI * ((i + 1) / M + 0.5) * (-1.0 if inverse else 1.0) for i in range(M // 2)]
    return [(F(math.cos(p)), F(math.sin(p))) for p in ph]


def c_mul(a, b):
    return (a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0])


def fftr(x):
    """One row of N real points -> N/2 + 1 bins."""
    x = np.ascontiguousarray(x, np.float32)
    M = len(x) // 2
    assert len(x) == 2 * M and M >= 1
    Z = O.fft(x.view(np.complex64)) if M > 1 else x.view(np.complex64).copy()
    zr, zi = Z.real.copy(), Z.imag.copy()
    tw = super_tw(M)
    fr, fi = np.zeros(M + 1, F), np.zeros(M + 1, F)
    fr[0], fr[M] = zr[0] + zi[0], zr[0] - zi[0]
    for k in range(1, M // 2 + 1):
        fpk, fpnk = (zr[k], zi[k]), (zr[M - k], -zi[M - k])
        f1 = (fpk[0] + fpnk[0], fpk[1] + fpnk[1])
        f2 = (fpk[0] - fpnk[0], fpk[1] - fpnk[1])
        w = c_mul(f2, tw[k - 1])
        fr[k], fi[k] = (f1[0] + w[0]) * HALF, (f1[1] + w[1]) * HALF
        fr[M - k], fi[M - k] = (f1[0] - w[0]) * HALF, (w[1] - f1[1]) * HALF
    out = np.empty(M + 1, np.complex64)
    out.real, out.imag = fr, fi
    return out


def fftri(f):
    """One row of M + 1 bins -> 2 M real points, unnormalised."""
    f = np.ascontiguousarray(f, np.complex64)
    M = len(f) - 1
    assert M >= 1
    fr, fi = f.real.copy(), f.imag.copy()
    tw = super_tw(M, inverse=True)
    tr, ti = np.zeros(M, F), np.zeros(M, F)
    tr[0], ti[0] = fr[0] + fr[M], fr[0] - fr[M]
    for k in range(1, M // 2 + 1):
        fk, fnkc = (fr[k], fi[k]), (fr[M - k], -fi[M - k])
        fek = (fk[0] + fnkc[0], fk[1] + fnkc[1])
        tmp = (fk[0] - fnkc[0], fk[1] - fnkc[1])
        fok = c_mul(tmp, tw[k - 1])
        tr[k], ti[k] = fek[0] + fok[0], fek[1] + fok[1]
        tr[M - k], ti[M - k] = fek[0] - fok[0], -(fek[1] - fok[1])
    T = np.empty(M, np.complex64)
    T.real, T.imag = tr, ti
    out = O.fft(T, inverse=True) if M > 1 else T
    return np.ascontiguousarray(out).view(np.float32).copy()


def fftr_rows(x, N):
    x = np.ascontiguousarray(x, np.float32).reshape(-1, N)
    return np.stack([fftr(r) for r in x])


def fftri_rows(f, N):
    f = np.ascontiguousarray(f, np.complex64).reshape(-1, N // 2 + 1)
    return np.stack([fftri(r) for r in f])
