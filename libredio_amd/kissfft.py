"""Mirror of the reference's kissfft crate (src/kissfft/src/kissfft.rs) over libkissfft.so.

`fft(pin, cout, block_size, inv)` keeps the reference block's signature (kissfft.rs:18): it owns one
cfg for its life (:19), asserts every message is exactly block_size long (:24), and sends a freshly
allocated output per message (:21-27).  Channels are anything with get()/put() (queue.Queue); a
`None` message ends the block (the reference loops until its channel hangs up and panics).
"""
import ctypes as C

import numpy as np

from . import kisslib


class Cfg:
    """kiss_fft_alloc(nfft, inverse, NULL, NULL) (kissfft.rs:19)."""

    def __init__(self, nfft, inverse=0):
        self.nfft = int(nfft)
        self._cfg = kisslib().kiss_fft_alloc(self.nfft, int(inverse), None, None)
        if not self._cfg:
            raise RuntimeError(f"kiss_fft_alloc({nfft}) failed (no HIP device or bad size)")

    def __call__(self, din):
        """kiss_fft(cfg, fin, fout) (kissfft.rs:26): host complex64 in, new host complex64 out."""
        din = np.ascontiguousarray(din, dtype=np.complex64)
        assert len(din) == self.nfft, "din.len() == block_size (kissfft.rs:24)"
        fout = np.empty(self.nfft, np.complex64)
        kisslib().kiss_fft(self._cfg, din.ctypes.data_as(C.c_void_p), fout.ctypes.data_as(C.c_void_p))
        return fout

    def close(self):
        if self._cfg:
            kisslib().kiss_fft_free(self._cfg)
            self._cfg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RealCfg:
    """kiss_fftr_alloc(nfft, inverse, NULL, NULL): nfft real points (even); a forward cfg maps nfft float32 to nfft/2 + 1 complex64
    (kiss_fftr), an inverse cfg the reverse, unnormalised (kiss_fftri)."""

    def __init__(self, nfft, inverse=0):
        self.nfft, self.inverse = int(nfft), int(bool(inverse))
        self._cfg = kisslib().kiss_fftr_alloc(self.nfft, self.inverse, None, None)
        if not self._cfg:
            raise RuntimeError(f"kiss_fftr_alloc({nfft}) failed (no HIP device, or an odd size)")

    def __call__(self, din):
        """kiss_fftr(cfg, timedata, freqdata) or kiss_fftri(cfg, freqdata, timedata): host in, new host array out."""
        nbins = self.nfft // 2 + 1
        if self.inverse:
            din = np.ascontiguousarray(din, dtype=np.complex64)
            assert len(din) == nbins, "din.len() == block_size / 2 + 1"
            out = np.empty(self.nfft, np.float32)
            kisslib().kiss_fftri(self._cfg, din.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        else:
            din = np.ascontiguousarray(din, dtype=np.float32)
            assert len(din) == self.nfft, "din.len() == block_size"
            out = np.empty(nbins, np.complex64)
            kisslib().kiss_fftr(self._cfg, din.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        return out

    def close(self):
        if self._cfg:
            kisslib().kiss_fftr_free(self._cfg)
            self._cfg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def fftr(pin, cout, block_size, inv):
    """The real-input twin of fft(): one RealCfg for the block's life, one message of block_size real samples (forward) or
    block_size / 2 + 1 bins (inverse) per transform; `None` ends the block."""
    cfg = RealCfg(block_size, inv)
    try:
        while True:
            din = pin.get()
            if din is None:
                break
            cout.put(cfg(din))
    finally:
        cfg.close()


def fft(pin, cout, block_size, inv):
    """kissfft::fft(pin, cout, block_size, inv) (kissfft.rs:18-31)."""
    cfg = Cfg(block_size, inv)
    try:
        while True:
            din = pin.get()
            if din is None:
                break
            cout.put(cfg(din))
    finally:
        cfg.close()
        kisslib().kiss_fft_cleanup()
