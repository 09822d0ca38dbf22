"""Device-resident plans of include/redio.h driven from torch tensors (torch = device memory and
streams only).  Inputs/outputs are torch CUDA tensors; kernels are enqueued on torch's current
stream, nothing synchronises."""
import ctypes as C
import threading

import numpy as np

from . import REDIO_FIR_COMPLEX, REDIO_FIR_FUSED, REDIO_PFB_OS_BLOCK, REDIO_PFB_PSPEC_BLOCK, check, lib, redio_msg

_pf = C.POINTER(C.c_float)


_tls = threading.local()  # capturing: how many Graph captures this thread has open
_deferred = []             # (destroy function, handle) of plans finalised on a thread while it was capturing


def _destroy_deferred():
    while _deferred and not getattr(_tls, "capturing", 0):
        fn, h = _deferred.pop()
        getattr(lib(), fn)(h)


def _safe_destroy(fn, h):
    """Plan destructors also run at interpreter shutdown, when module globals may already be gone.  And they run wherever the
    collector finds a plan that sat in a reference cycle (a caught exception's traceback keeps its frame's locals): inside a Graph
    capture on this thread the destroy would free device memory, which HIP refuses on a capturing thread and answers by invalidating
    the capture -- so it waits for the capture's end."""
    try:
        if getattr(_tls, "capturing", 0):
            _deferred.append((fn, h))
            return
        getattr(lib(), fn)(h)
        _destroy_deferred()
    except Exception:
        pass


def current_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev_ptr(t):
    assert t.is_cuda and t.is_contiguous(), "device-resident, contiguous tensors only"
    return C.c_void_p(t.data_ptr())


def _taps(taps):
    t = np.ascontiguousarray(taps, dtype=np.float32)
    return t, t.ctypes.data_as(_pf)


class Fir:
    """redio_fir_*: valid-mode FIR with the fold order of dsputils::convolve (dsputils.rs:30-32),
    optional decimation, real (float32) or interleaved complex (complex64) streams."""

    def __init__(self, taps, decim=1, complex_input=True, fused=False):
        t, p = _taps(taps)
        self.ntaps, self.decim, self.complex_input = len(t), int(decim), complex_input
        flags = (REDIO_FIR_COMPLEX if complex_input else 0) | (REDIO_FIR_FUSED if fused else 0)
        self._h = C.c_void_p()
        check(lib().redio_fir_create(C.byref(self._h), p, len(t), self.decim, flags), "fir_create")

    def nout(self, n_in):
        return lib().redio_fir_nout(self._h, n_in)

    def __call__(self, x, out=None):
        import torch
        want = torch.complex64 if self.complex_input else torch.float32
        assert x.dtype == want, f"expected {want}"
        n = self.nout(x.numel())
        if out is None:
            out = torch.empty(n, dtype=want, device=x.device)
        assert out.numel() >= n
        check(lib().redio_fir_enqueue(self._h, _dev_ptr(x), x.numel(), _dev_ptr(out), current_stream()), "fir_enqueue")
        return out[:n]

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_fir_destroy", self._h)
            self._h = None


class Ddc:
    """redio_ddc_*: the tuner -- kpn::mul_vecs (kpn.rs:198-203) by the periodic oscillator table `osc` (complex64, any period up to
    REDIO_DDC_MAX_PERIOD; dsputils.osc_table makes one), then the FIR of dsputils::convolve (dsputils.rs:30-32) with decimation, in one
    kernel; bit for bit Fir(taps, decim)(x * osc tiled from `first`).  complex64 in (or uint8 I/Q bytes through from_bytes), complex64 out."""

    def __init__(self, osc, taps, decim=1, fused=False):
        t, p = _taps(taps)
        w = np.ascontiguousarray(osc, dtype=np.complex64).reshape(-1)
        self.ntaps, self.decim, self.complex_input = len(t), int(decim), True
        self._h = C.c_void_p()
        check(lib().redio_ddc_create(C.byref(self._h), w.view(np.float32).ctypes.data_as(_pf), len(w), p, len(t), self.decim,
                                     REDIO_FIR_FUSED if fused else 0), "ddc_create")

    def nout(self, n_in):
        return lib().redio_ddc_nout(self._h, n_in)

    @property
    def route(self):
        """redio_ddc_route: 1 the specialised tiled kernel, 2 the any-taps chunked one, 3 the direct one."""
        return lib().redio_ddc_route(self._h)

    @property
    def period(self):
        return lib().redio_ddc_period(self._h)

    def _run(self, fn, x, nsamp, count, first, out):
        import torch
        n = self.nout(nsamp)
        if out is None:
            out = torch.empty(n, dtype=torch.complex64, device=x.device)
        assert out.dtype == torch.complex64 and out.numel() >= n
        check(getattr(lib(), fn)(self._h, _dev_ptr(x), count, int(first), _dev_ptr(out), current_stream()), fn[6:])
        return out[:n]

    def __call__(self, x, first=0, out=None):
        """`first`: the stream index of x[0] (the table entry of sample n is osc[(first + n) % period])."""
        import torch
        assert x.dtype == torch.complex64
        return self._run("redio_ddc_enqueue", x, x.numel(), x.numel(), first, out)

    def from_bytes(self, raw, first=0, out=None):
        """redio_ddc_enqueue_u8: the receiver's interleaved u8 I/Q bytes (rtlsdr.rs:159-162); bitfount.data_to_samples(raw) through
        __call__, bit for bit."""
        import torch
        assert raw.dtype == torch.uint8 and raw.numel() % 2 == 0
        return self._run("redio_ddc_enqueue_u8", raw, raw.numel() // 2, raw.numel(), first, out)

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_ddc_destroy", self._h)
            self._h = None


class Upfirdn:
    """redio_upfirdn_*: the rational resampler -- up by `up`, the FIR of dsputils::convolve (dsputils.rs:30-32), down by `down`, as a
    polyphase FIR over the original samples: bit for bit the fold over the taps that meet a sample, the stuffed zeros skipped.
    float32 streams, or complex64 with complex_input."""

    def __init__(self, taps, up, down, complex_input=False, fused=False):
        t, p = _taps(taps)
        self.ntaps, self.up, self.down, self.complex_input = len(t), int(up), int(down), complex_input
        flags = (REDIO_FIR_COMPLEX if complex_input else 0) | (REDIO_FIR_FUSED if fused else 0)
        self._h = C.c_void_p()
        check(lib().redio_upfirdn_create(C.byref(self._h), p, len(t), self.up, self.down, flags), "upfirdn_create")

    def nout(self, n_in):
        return lib().redio_upfirdn_nout(self._h, n_in)

    @property
    def route(self):
        """redio_upfirdn_route: 1 the phase-walking tiled kernel, 2 the direct one."""
        return lib().redio_upfirdn_route(self._h)

    @property
    def period_out(self):
        """U' = up / gcd(up, down): outputs per period"""
        return lib().redio_upfirdn_period_out(self._h)

    @property
    def period_in(self):
        """D' = down / gcd(up, down): new samples per period"""
        return lib().redio_upfirdn_period_in(self._h)

    @property
    def window(self):
        """Wp: samples one period reads"""
        return lib().redio_upfirdn_window(self._h)

    def __call__(self, x, out=None):
        import torch
        want = torch.complex64 if self.complex_input else torch.float32
        assert x.dtype == want, f"expected {want}"
        n = self.nout(x.numel())
        if out is None:
            out = torch.empty(n, dtype=want, device=x.device)
        assert out.dtype == want and out.numel() >= n
        check(lib().redio_upfirdn_enqueue(self._h, _dev_ptr(x), x.numel(), _dev_ptr(out), current_stream()), "upfirdn_enqueue")
        return out[:n]

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_upfirdn_destroy", self._h)
            self._h = None


class DdcUpfirdn:
    """redio_ddc_upfirdn_*: the tuned resampler -- kpn::mul_vecs (kpn.rs:198-203) by the periodic oscillator table `osc` (as Ddc's), then
    the rational resampler (as Upfirdn's: up by `up`, the FIR of dsputils::convolve, dsputils.rs:30-32, down by `down`) in one kernel;
    bit for bit Upfirdn(taps, up, down, complex_input=True)(x * osc tiled from `first`).  complex64 in (or uint8 I/Q bytes through
    from_bytes), complex64 out."""

    def __init__(self, osc, taps, up, down, fused=False):
        t, p = _taps(taps)
        w = np.ascontiguousarray(osc, dtype=np.complex64).reshape(-1)
        self.ntaps, self.up, self.down, self.complex_input = len(t), int(up), int(down), True
        self._h = C.c_void_p()
        check(lib().redio_ddc_upfirdn_create(C.byref(self._h), w.view(np.float32).ctypes.data_as(_pf), len(w), p, len(t), self.up, self.down,
                                             REDIO_FIR_FUSED if fused else 0), "ddc_upfirdn_create")

    def nout(self, n_in):
        return lib().redio_ddc_upfirdn_nout(self._h, n_in)

    @property
    def route(self):
        """redio_ddc_upfirdn_route: 1 the phase-walking tiled kernel, 2 the direct one."""
        return lib().redio_ddc_upfirdn_route(self._h)

    @property
    def period(self):
        """the oscillator's"""
        return lib().redio_ddc_upfirdn_period(self._h)

    @property
    def period_out(self):
        """U' = up / gcd(up, down): outputs per period"""
        return lib().redio_ddc_upfirdn_period_out(self._h)

    @property
    def period_in(self):
        """D' = down / gcd(up, down): new samples per period"""
        return lib().redio_ddc_upfirdn_period_in(self._h)

    @property
    def window(self):
        """Wp: samples one period reads"""
        return lib().redio_ddc_upfirdn_window(self._h)

    def _run(self, fn, x, nsamp, count, first, out):
        import torch
        n = self.nout(nsamp)
        if out is None:
            out = torch.empty(n, dtype=torch.complex64, device=x.device)
        assert out.dtype == torch.complex64 and out.numel() >= n
        check(getattr(lib(), fn)(self._h, _dev_ptr(x), count, int(first), _dev_ptr(out), current_stream()), fn[6:])
        return out[:n]

    def __call__(self, x, first=0, out=None):
        """`first`: the stream index of x[0] (the table entry of sample n is osc[(first + n) % period])."""
        import torch
        assert x.dtype == torch.complex64
        return self._run("redio_ddc_upfirdn_enqueue", x, x.numel(), x.numel(), first, out)

    def from_bytes(self, raw, first=0, out=None):
        """redio_ddc_upfirdn_enqueue_u8: the receiver's interleaved u8 I/Q bytes (rtlsdr.rs:159-162); bitfount.data_to_samples(raw)
        through __call__, bit for bit."""
        import torch
        assert raw.dtype == torch.uint8 and raw.numel() % 2 == 0
        return self._run("redio_ddc_upfirdn_enqueue_u8", raw, raw.numel() // 2, raw.numel(), first, out)

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_ddc_upfirdn_destroy", self._h)
            self._h = None


class Fft:
    """redio_fft_*: batched kissfft::fft blocks (kissfft.rs:18-31), unnormalised."""

    def __init__(self, nfft, inverse=False):
        self.nfft = int(nfft)
        self._h = C.c_void_p()
        check(lib().redio_fft_create(C.byref(self._h), self.nfft, int(bool(inverse))), "fft_create")

    def reserve(self, nbatch):
        """redio_fft_reserve: the staging buffer of the sizes that need one, for calls of up to nbatch messages (before a graph capture)."""
        check(lib().redio_fft_reserve(self._h, nbatch), "fft_reserve")

    def __call__(self, x, out=None):
        import torch
        assert x.dtype == torch.complex64 and x.numel() % self.nfft == 0, "messages of exactly nfft samples"
        if out is None:
            out = torch.empty_like(x)
        check(lib().redio_fft_enqueue(self._h, _dev_ptr(x), _dev_ptr(out), x.numel() // self.nfft, current_stream()), "fft_enqueue")
        return out

    def enqueue_list(self, xs, outs=None):
        """redio_fft_enqueue_list: every tensor of `xs` is its own message of whole nfft-sample transforms, all in one launch
        (nfft 1024; other sizes one launch per message); the same bits as one call per message.  Returns the outputs."""
        import torch
        for x in xs:
            assert x.dtype == torch.complex64 and x.numel() % self.nfft == 0, "messages of whole nfft-sample transforms"
        if outs is None:
            outs = [torch.empty_like(x) for x in xs]
        assert len(outs) == len(xs) and all(o.numel() >= x.numel() for x, o in zip(xs, outs))
        msgs = (redio_msg * max(len(xs), 1))(*[redio_msg(_dev_ptr(x), x.numel() // self.nfft, _dev_ptr(o)) for x, o in zip(xs, outs)])
        check(lib().redio_fft_enqueue_list(self._h, msgs, len(xs), current_stream()), "fft_enqueue_list")
        return outs

    def strided(self, x, nbatch, in_stride, out=None):
        """redio_fft_enqueue_strided: block b is x[b*in_stride : b*in_stride + nfft] (overlapping when in_stride < nfft,
        the overlap-save framing); the outputs are packed."""
        import torch
        assert x.dtype == torch.complex64 and in_stride > 0 and (nbatch == 0 or (nbatch - 1) * in_stride + self.nfft <= x.numel())
        if out is None:
            out = torch.empty(nbatch * self.nfft, dtype=torch.complex64, device=x.device)
        check(lib().redio_fft_enqueue_strided(self._h, _dev_ptr(x), _dev_ptr(out), nbatch, in_stride, current_stream()), "fft_enqueue_strided")
        return out

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_fft_destroy", self._h)
            self._h = None


class Fftr:
    """redio_fftr_*: batched kiss_fftr (rows of nfft float32 -> rows of nfft/2 + 1 complex64) or, with inverse=True, kiss_fftri (the
    reverse, unnormalised).  nfft counts real points and is even."""

    def __init__(self, nfft, inverse=False):
        self.nfft, self.inverse = int(nfft), bool(inverse)
        self.nbins = self.nfft // 2 + 1
        self._h = C.c_void_p()
        check(lib().redio_fftr_create(C.byref(self._h), self.nfft, int(self.inverse)), "fftr_create")

    @property
    def is_fused(self):
        return bool(lib().redio_fftr_is_fused(self._h))

    def reserve(self, nbatch):
        check(lib().redio_fftr_reserve(self._h, nbatch), "fftr_reserve")

    def _sides(self):
        import torch
        if self.inverse:
            return torch.complex64, self.nbins, torch.float32, self.nfft
        return torch.float32, self.nfft, torch.complex64, self.nbins

    def __call__(self, x, out=None):
        import torch
        din, nin, dout, nout = self._sides()
        assert x.dtype == din and x.numel() % nin == 0, "whole rows of the plan's input side"
        nbatch = x.numel() // nin
        if out is None:
            out = torch.empty(nbatch * nout, dtype=dout, device=x.device)
        assert out.dtype == dout and out.numel() >= nbatch * nout
        check(lib().redio_fftr_enqueue(self._h, _dev_ptr(x), _dev_ptr(out), nbatch, current_stream()), "fftr_enqueue")
        return out

    def strided(self, x, nbatch, in_stride, out_stride=None, out=None):
        """redio_fftr_enqueue_strided: row b is x[b*in_stride : b*in_stride + row] (a forward in_stride < nfft gives overlapping
        frames) and lands at out[b*out_stride : ...]; strides count elements of their own side, out_stride defaults to packed rows."""
        import torch
        din, nin, dout, nout = self._sides()
        if out_stride is None:
            out_stride = nout
        assert x.dtype == din and in_stride > 0 and (nbatch == 0 or (nbatch - 1) * in_stride + nin <= x.numel())
        if out is None:
            out = torch.empty(max(nbatch - 1, 0) * out_stride + (nout if nbatch else 0), dtype=dout, device=x.device)
        assert out.dtype == dout and (nbatch == 0 or (nbatch - 1) * out_stride + nout <= out.numel())
        check(lib().redio_fftr_enqueue_strided(self._h, _dev_ptr(x), _dev_ptr(out), nbatch, in_stride, out_stride, current_stream()),
              "fftr_enqueue_strided")
        return out

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_fftr_destroy", self._h)
            self._h = None


class Chain:
    """redio_chain_*: FIR(ntaps, decimate) -> nfft-point forward FFT over consecutive blocks."""

    def __init__(self, taps, decim, nfft, fused=True):
        t, p = _taps(taps)
        self.ntaps, self.decim, self.nfft = len(t), int(decim), int(nfft)
        self._h = C.c_void_p()
        check(lib().redio_chain_create(C.byref(self._h), p, len(t), self.decim, self.nfft,
                                       REDIO_FIR_FUSED if fused else 0), "chain_create")

    def nblocks(self, n_in):
        return lib().redio_chain_nblocks(self._h, n_in)

    @property
    def is_fused(self):
        return bool(lib().redio_chain_is_fused(self._h))

    def set_unfused(self, unfused):
        check(lib().redio_chain_set_unfused(self._h, int(bool(unfused))), "chain_set_unfused")

    def reserve(self, n_in):
        """Size the two-kernel path's intermediate up front (enqueue then never allocates)."""
        check(lib().redio_chain_reserve(self._h, int(n_in)), "chain_reserve")

    def blocks_per_wave(self, nblocks):
        """redio_chain_blocks_per_wave: consecutive blocks one wavefront of the fused launch over `nblocks` blocks owns (0: two kernels)."""
        return lib().redio_chain_blocks_per_wave(self._h, int(nblocks))

    def launch_waves(self, nblocks):
        """redio_chain_launch_waves: wavefronts of the fused launch over `nblocks` blocks (0: two kernels)."""
        return lib().redio_chain_launch_waves(self._h, int(nblocks))

    @property
    def kernel_name(self):
        """redio_chain_kernel_name: the fused kernel as rocprofv3 names it, spaces removed (None for a two-kernel plan)."""
        n = lib().redio_chain_kernel_name(self._h)
        return n.decode() if n else None

    def set_debug_stamps(self, buf):
        """Diagnostic per-wave stamps of this plan's fused launches into `buf` (int64 CUDA tensor, 4 per wave: size it with
        4 * launch_waves(nblocks); wavefronts beyond its capacity leave no stamp); None = off."""
        if buf is None:
            check(lib().redio_chain_set_debug_stamps(self._h, None, 0), "chain_set_debug_stamps")
        else:
            check(lib().redio_chain_set_debug_stamps(self._h, C.c_void_p(buf.data_ptr()), buf.numel() // 4), "chain_set_debug_stamps")

    def __call__(self, x, out=None):
        import torch
        assert x.dtype == torch.complex64
        nb = self.nblocks(x.numel())
        if out is None:
            out = torch.empty((nb, self.nfft), dtype=torch.complex64, device=x.device)
        assert out.numel() >= nb * self.nfft
        check(lib().redio_chain_enqueue(self._h, _dev_ptr(x), x.numel(), _dev_ptr(out), current_stream()), "chain_enqueue")
        return out

    def enqueue_list(self, xs, outs=None):
        """redio_chain_enqueue_list: every cf32 tensor of `xs` is its own message, all in one launch on a fused plan; the same bits as
        one call per message.  Returns the outputs, (nblocks, nfft) each."""
        import torch
        nbs = []
        for x in xs:
            assert x.dtype == torch.complex64
            nbs.append(self.nblocks(x.numel()))
        if outs is None:
            outs = [torch.empty((nb, self.nfft), dtype=torch.complex64, device=x.device) for x, nb in zip(xs, nbs)]
        assert len(outs) == len(xs) and all(o.numel() >= nb * self.nfft for o, nb in zip(outs, nbs))
        msgs = (redio_msg * max(len(xs), 1))(*[redio_msg(_dev_ptr(x), x.numel(), _dev_ptr(o)) for x, o in zip(xs, outs)])
        check(lib().redio_chain_enqueue_list(self._h, msgs, len(xs), current_stream()), "chain_enqueue_list")
        return outs

    def reserve_u8(self, nbytes):
        """Size what from_bytes needs beyond the one-kernel form (other shapes, unaligned bytes) for messages of up to nbytes bytes."""
        check(lib().redio_chain_reserve_u8(self._h, int(nbytes)), "chain_reserve_u8")

    def from_bytes(self, raw, out=None):
        """redio_chain_enqueue_u8: the receiver's interleaved u8 I/Q bytes (rtlsdr::data_to_samples, rtlsdr.rs:159-162)
        straight into the chain; the spectra of bitfount.data_to_samples(raw) followed by this plan, bit for bit."""
        import torch
        assert raw.dtype == torch.uint8 and raw.numel() % 2 == 0
        nb = self.nblocks(raw.numel() // 2)
        if out is None:
            out = torch.empty((nb, self.nfft), dtype=torch.complex64, device=raw.device)
        assert out.numel() >= nb * self.nfft
        check(lib().redio_chain_enqueue_u8(self._h, _dev_ptr(raw), raw.numel(), _dev_ptr(out), current_stream()), "chain_enqueue_u8")
        return out

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_chain_destroy", self._h)
            self._h = None


class Stream:
    """redio_{fir,chain,pfb,ovsave,ovsave_real,pspec,pspec_real,pfb_pspec,ddc,upfirdn,ddc_upfirdn,pfb_synth,pfb_os,pfb_os_synth}_stream_*: a plan fed as a STREAM with the history carried on the device, so that any
    segmentation of the input gives the bits of one stateless call on the whole stream (the stateless plans keep the
    reference's per-message semantics, dsputils.rs:30-32).  `plan` is a Fir, Chain, Channelizer, OverlapSave, OverlapSaveReal, PowerSpectrum
    (complex64 in, float32 rows out), PowerSpectrumReal (float32 in, float32 rows out), PolyphaseSpectrum (complex64 in, float32 rows
    of nchan out), Ddc (the tuner: the oscillator's phase is carried with the history) or Upfirdn (whole periods of period_out samples
    from the window that starts at a multiple of period_in samples of the stream), a DdcUpfirdn (the tuned resampler: the resampler's whole
    periods with the oscillator's phase carried as the tuner's is), or a Synthesizer (channel values in, whole rows of
    nchan samples of the one stream out: see SynthesizerStream), or an OversampledChannelizer (whole rows of nchan channels, the running
    row index carried with the samples: see OversampledChannelizerStream), or an OversampledSynthesizer (channel values in, whole hops of
    the one stream out: see OversampledSynthesizerStream)."""

    def __init__(self, plan, u8=False):
        """u8=True (Chain, Channelizer, PowerSpectrum, PolyphaseSpectrum, Ddc and DdcUpfirdn): the stream arrives as the receiver's interleaved u8 I/Q
        bytes (uint8 tensors, two bytes per sample; redio_{chain,pfb,pspec,pfb_pspec,ddc,ddc_upfirdn}_stream_create_u8)."""
        kind = {Fir: "fir", Chain: "chain", Ddc: "ddc", Upfirdn: "upfirdn", DdcUpfirdn: "ddc_upfirdn"}.get(type(plan)) or {"Channelizer": "pfb", "OverlapSave": "ovsave", "OverlapSaveReal": "ovsave_real", "PowerSpectrum": "pspec", "PowerSpectrumReal": "pspec_real", "PolyphaseSpectrum": "pfb_pspec", "Synthesizer": "pfb_synth", "OversampledChannelizer": "pfb_os", "OversampledSynthesizer": "pfb_os_synth"}[type(plan).__name__]
        assert not u8 or kind in ("chain", "pfb", "pspec", "pfb_pspec", "ddc", "ddc_upfirdn")
        self._kind, self._plan, self._u8 = kind, plan, bool(u8)          # the plan must outlive the stream handle
        self._h = C.c_void_p()
        check(getattr(lib(), f"redio_{kind}_stream_create" + ("_u8" if u8 else ""))(C.byref(self._h), plan._h), f"{kind}_stream_create")

    def _f(self, name):
        return getattr(lib(), f"redio_{self._kind}_stream_{name}")

    def nout(self, n_new):
        return self._f("nout")(self._h, int(n_new))

    @property
    def pending(self):
        return self._f("pending")(self._h)

    def reset(self):
        check(self._f("reset")(self._h), "stream_reset")

    @property
    def index(self):
        """redio_ddc_stream_index / redio_ddc_upfirdn_stream_index (a Ddc or DdcUpfirdn stream only): the stream index of the next new sample, which is the oscillator's phase."""
        return self._f("index")(self._h)

    def __call__(self, x, out=None):
        """Feed the next piece of the stream; returns the output samples that became computable (flat tensor; the
        chain's are whole spectra of nfft samples, the channelizer's whole rows of nchan samples)."""
        import torch
        real = self._kind in ("ovsave_real", "pspec_real") or (self._kind in ("fir", "upfirdn") and not self._plan.complex_input)
        want = torch.float32 if real else torch.complex64
        if self._u8:
            assert x.dtype == torch.uint8 and x.numel() % 2 == 0, "expected an even number of uint8 bytes"
            nsamp = x.numel() // 2
        else:
            assert x.dtype == want, f"expected {want}"
            nsamp = x.numel()
        n = self.nout(nsamp)
        if out is None:
            out = torch.empty(max(n, 1), dtype=torch.float32 if self._kind in ("pspec", "pfb_pspec") else want, device=x.device)
        assert out.numel() >= n
        got = C.c_size_t(0)
        check(self._f("enqueue")(self._h, _dev_ptr(x) if x.numel() else None, nsamp, _dev_ptr(out), C.byref(got), current_stream()),
              f"{self._kind}_stream_enqueue")
        assert got.value == n
        return out[:n]

    def __del__(self, _safe_destroy=_safe_destroy):
        if getattr(self, "_h", None):
            _safe_destroy(f"redio_{self._kind}_stream_destroy", self._h)
            self._h = None


class Src:
    """redio_src_*: nchan independent mono streams through the libsamplerate-style sinc converter
    (samplerate.rs:59-87 semantics per stream), device-resident rows [nchan][frames]."""

    EXACT, FAST, EPOCHS = 0, 1, 2

    def __init__(self, nchan, converter=1, mode=0):
        self.nchan = int(nchan)
        self._h = C.c_void_p()
        check(lib().redio_src_create(C.byref(self._h), int(converter), self.nchan), "src_create")
        if mode:
            self.set_mode(mode)

    def set_mode(self, mode):
        """EXACT (bit-identical, default) / FAST (f32 polyphase for uniform-phase calls) / EPOCHS
        (EXACT, one launch per buffer refill)."""
        check(lib().redio_src_set_mode(self._h, int(mode)), "src_set_mode")

    def process(self, x, ratio, output_frames=None, end_of_input=False):
        """x: float32 CUDA tensor [nchan, frames]. Returns (out[nchan, gen], input_frames_used)."""
        import torch
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] == self.nchan and x.is_contiguous()
        frames = x.shape[1]
        cap = int(ratio * frames + 1.0) if output_frames is None else int(output_frames)
        out = torch.empty((self.nchan, max(cap, 1)), dtype=torch.float32, device=x.device)
        used, gen = C.c_long(0), C.c_long(0)
        rc = lib().redio_src_process(self._h, _dev_ptr(x), frames, x.stride(0), _dev_ptr(out), cap, out.stride(0),
                                     float(ratio), int(bool(end_of_input)), C.byref(used), C.byref(gen), current_stream())
        check(rc, "src_process")
        return out[:, : gen.value], used.value

    def enqueue(self, x, ratio, out=None, output_frames=None, packed=False):
        """redio_src_enqueue: process() without end_of_input in stream order -- a uniform-phase call (constant ratio, integer 1/ratio)
        after the first at its ratio only launches, nothing synchronises.  x: float32 CUDA tensor [nchan, frames], rows contiguous
        (any row stride).  out: float32 CUDA tensor of at least nchan * capacity elements (allocated when None).  Returns
        (out[nchan, gen], input_frames_used, gen); with packed=True the rows are written back to back and the result is a
        contiguous [nchan, gen] view of the start of `out`."""
        import torch
        assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] == self.nchan and x.is_cuda and (x.shape[1] <= 1 or x.stride(1) == 1)
        frames = x.shape[1]
        cap = int(ratio * frames + 1.0) if output_frames is None else int(output_frames)
        if out is None:
            out = torch.empty((self.nchan, max(cap, 1)), dtype=torch.float32, device=x.device)
        assert out.dtype == torch.float32 and out.is_cuda and out.is_contiguous() and out.numel() >= self.nchan * cap
        stride = 0 if packed else (out.stride(0) if out.dim() == 2 else max(cap, 1))
        used, gen = C.c_long(0), C.c_long(0)
        rc = lib().redio_src_enqueue(self._h, C.c_void_p(x.data_ptr()), frames, x.stride(0), C.c_void_p(out.data_ptr()), cap, stride,
                                     float(ratio), C.byref(used), C.byref(gen), current_stream())
        check(rc, "src_enqueue")
        g = gen.value
        if packed:
            return out.reshape(-1)[: self.nchan * g].view(self.nchan, g), used.value, g
        if out.dim() == 2:
            return out[:, :g], used.value, g
        return out.reshape(-1)[: self.nchan * stride].view(self.nchan, stride)[:, :g], used.value, g

    def enqueue_counts(self):
        """(calls of enqueue() that only launched, calls that ran the synchronising path)."""
        a, b = C.c_long(0), C.c_long(0)
        check(lib().redio_src_enqueue_counts(self._h, C.byref(a), C.byref(b)), "src_enqueue_counts")
        return a.value, b.value

    def reset(self):
        check(lib().redio_src_reset(self._h), "src_reset")

    def path_counts(self):
        """(epochs through the periodic-phase kernel, epochs through the general per-tap kernel) so far."""
        a, b = C.c_long(0), C.c_long(0)
        check(lib().redio_src_path_counts(self._h, C.byref(a), C.byref(b)), "src_path_counts")
        return a.value, b.value

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_src_destroy", self._h)
            self._h = None


class Graph:
    """redio_graph_*: record the enqueue calls issued inside the `with` block on a side stream and replay
    them with one submission (launch-bound pipelines of many small messages).  Allocate every output
    before entering and run the sequence once un-captured first.

        g = Graph()
        with g:                      # torch's current stream is the capture stream inside the block
            for i in range(64):
                fir(x[i], out=y[i]); fft(y[i], out=z[i])
        g.launch(); g.launch()
    """

    def __init__(self):
        import torch
        self.stream = torch.cuda.Stream()
        self._g = C.c_void_p()
        self._ctx = None

    def __enter__(self):
        import torch
        self.stream.wait_stream(torch.cuda.current_stream())
        self._ctx = torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        check(lib().redio_graph_begin(C.c_void_p(self.stream.cuda_stream)), "graph_begin")
        _tls.capturing = getattr(_tls, "capturing", 0) + 1  # _safe_destroy: plans finalised on this thread wait for the capture's end
        return self

    def __exit__(self, et, ev, tb):
        try:
            rc = lib().redio_graph_end(C.c_void_p(self.stream.cuda_stream), C.byref(self._g))
        finally:
            _tls.capturing -= 1
        _destroy_deferred()
        self._ctx.__exit__(et, ev, tb)
        self._ctx = None
        if et is None:
            check(rc, "graph_end")
        return False

    def launch(self, stream=None):
        """Replay on `stream` (default: torch's current stream)."""
        check(lib().redio_graph_launch(self._g, current_stream() if stream is None else C.c_void_p(stream.cuda_stream)), "graph_launch")

    def __del__(self, _safe_destroy=_safe_destroy):
        if getattr(self, "_g", None):
            _safe_destroy("redio_graph_destroy", self._g)
            self._g = None


def synth_iq(seed, first, n, device="cuda"):
    """Hash-generated cf32 IQ in [-1,1), generated on the device."""
    import torch
    out = torch.empty(n, dtype=torch.complex64, device=device)
    check(lib().redio_synth_iq(_dev_ptr(out), seed, first, n, current_stream()), "synth_iq")
    return out


def synth_f32(seed, first, n, device="cuda"):
    import torch
    out = torch.empty(n, dtype=torch.float32, device=device)
    check(lib().redio_synth_f32(_dev_ptr(out), seed, first, n, current_stream()), "synth_f32")
    return out


def rows_to_planes(rows, out=None, plane_stride=None):
    """redio_rows_to_planes_c32: complex64 [nrows, nchan] (the channelizer's rows) -> float32 [2*nchan, plane_stride], plane 2c = Re and
    plane 2c + 1 = Im of channel c in its first nrows entries -- Src.enqueue's rows for 2*nchan mono streams."""
    import torch
    assert rows.dtype == torch.complex64 and rows.dim() == 2
    nrows, nchan = rows.shape
    stride = nrows if plane_stride is None else int(plane_stride)
    if out is None:
        out = torch.empty((2 * nchan, stride), dtype=torch.float32, device=rows.device)
    assert out.dtype == torch.float32 and out.numel() >= 2 * nchan * stride
    check(lib().redio_rows_to_planes_c32(_dev_ptr(rows), nrows, nchan, _dev_ptr(out), stride, current_stream()), "rows_to_planes")
    return out


def planes_to_rows(planes, nrows=None, out=None):
    """redio_planes_to_rows_c32, the inverse: float32 [2*nchan, plane_stride] -> complex64 [nrows, nchan] (nrows: plane_stride when None)."""
    import torch
    assert planes.dtype == torch.float32 and planes.dim() == 2 and planes.shape[0] % 2 == 0
    nchan, stride = planes.shape[0] // 2, planes.shape[1]
    nrows = stride if nrows is None else int(nrows)
    if out is None:
        out = torch.empty((nrows, nchan), dtype=torch.complex64, device=planes.device)
    assert out.dtype == torch.complex64 and out.numel() >= nrows * nchan
    check(lib().redio_planes_to_rows_c32(_dev_ptr(planes), stride, nrows, nchan, _dev_ptr(out), current_stream()), "planes_to_rows")
    return out


class Channelizer:
    """redio_pfb_*: polyphase channelizer (BASELINE.json configs[3]): branch FIRs with the dsputils fold + kissfft
    across branches.  64 channels with 4 / 8 / 16 taps per branch run one fused kernel; any other shape runs the
    branch filters and the plan's transform as two passes.  out[row][channel], or [group][row][nchan/ngroups] for
    the multi-GPU regrouping (see channelizer_all_to_all)."""

    def __init__(self, proto, nchan=64, taps_per_branch=16, fused=True):
        t, p = _taps(proto)
        assert len(t) == nchan * taps_per_branch
        self.nchan, self.taps_per_branch = int(nchan), int(taps_per_branch)
        self._h = C.c_void_p()
        check(lib().redio_pfb_create(C.byref(self._h), p, self.nchan, self.taps_per_branch,
                                     REDIO_FIR_FUSED if fused else 0), "pfb_create")

    def nrows(self, n_in):
        return lib().redio_pfb_nrows(self._h, n_in)

    def __call__(self, x, ngroups=1, out=None):
        import torch
        assert x.dtype == torch.complex64
        rows = self.nrows(x.numel())
        if out is None:
            shape = (rows, self.nchan) if ngroups == 1 else (ngroups, rows, self.nchan // ngroups)
            out = torch.empty(shape, dtype=torch.complex64, device=x.device)
        check(lib().redio_pfb_enqueue(self._h, _dev_ptr(x), x.numel(), _dev_ptr(out), int(ngroups), current_stream()), "pfb_enqueue")
        return out

    def reserve(self, n_in, ngroups=1, two_pass=False):
        """redio_pfb_reserve / redio_pfb_reserve_two_pass: plan scratch for inputs of up to n_in samples (so that a call never allocates,
        e.g. inside a Graph); two_pass: also for the one-kernel shapes, whose fall-back for an output that is not 16-byte aligned needs it."""
        f = lib().redio_pfb_reserve_two_pass if two_pass else lib().redio_pfb_reserve
        check(f(self._h, int(n_in), int(ngroups)), "pfb_reserve")

    def from_bytes(self, raw, ngroups=1, out=None):
        """redio_pfb_enqueue_u8: the receiver's interleaved u8 I/Q bytes (rtlsdr::data_to_samples, rtlsdr.rs:159-162) straight
        into the channelizer; the rows of bitfount.data_to_samples(raw) followed by this plan, bit for bit."""
        import torch
        assert raw.dtype == torch.uint8 and raw.numel() % 2 == 0
        rows = self.nrows(raw.numel() // 2)
        if out is None:
            shape = (rows, self.nchan) if ngroups == 1 else (ngroups, rows, self.nchan // ngroups)
            out = torch.empty(shape, dtype=torch.complex64, device=raw.device)
        check(lib().redio_pfb_enqueue_u8(self._h, _dev_ptr(raw), raw.numel(), _dev_ptr(out), int(ngroups), current_stream()), "pfb_enqueue_u8")
        return out

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_pfb_destroy", self._h)
            self._h = None


def channelizer_all_to_all(grouped, group=None):
    """The one exchange step of the time-sharded channelizer: every rank holds
    grouped[g] = [its rows][channels of rank g]; after the all-to-all rank g holds
    [all rows, in rank (= time) order][its channels].  Rows per rank may differ (ragged split sizes).
    Works with any torch.distributed backend (nccl = RCCL over xGMI on the GPU box, gloo in the CPU tests)."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    assert grouped.shape[0] == world
    my_rows, cpg = grouped.shape[1], grouped.shape[2]
    rows = [torch.zeros(1, dtype=torch.int64, device=grouped.device) for _ in range(world)]
    dist.all_gather(rows, torch.tensor([my_rows], dtype=torch.int64, device=grouped.device), group=group)
    rows = [int(r) for r in rows]
    send = torch.view_as_real(grouped.contiguous()).reshape(world * my_rows, cpg * 2)
    recv = torch.empty((sum(rows), cpg * 2), dtype=send.dtype, device=send.device)
    dist.all_to_all_single(recv, send, output_split_sizes=rows, input_split_sizes=[my_rows] * world, group=group)
    return torch.view_as_complex(recv.reshape(sum(rows), cpg, 2))


class Comm:
    """redio_comm_* / redio_pfb_exchange: the channelizer's regrouping step through the C ABI (RCCL ncclSend/ncclRecv
    inside one group) -- what a Rust or C++ kpn host calls.  channelizer_all_to_all above is the torch.distributed
    twin (and the only form the gloo CPU tests can run)."""

    def __init__(self, handle, rank, size):
        self._h, self.rank, self.size = handle, rank, size

    @classmethod
    def from_torch_distributed(cls, group=None):
        """One rank per process under torch.distributed.run: rank 0 makes the RCCL id, the process group carries the
        128 bytes to the others (any backend), every rank joins on its current device."""
        import torch.distributed as dist
        rank, world = dist.get_rank(group), dist.get_world_size(group)
        buf = C.create_string_buffer(128)
        if rank == 0:
            check(lib().redio_comm_unique_id(buf), "comm_unique_id")
        box = [buf.raw]
        dist.broadcast_object_list(box, src=0, group=group)
        h = C.c_void_p()
        check(lib().redio_comm_init_rank(C.byref(h), world, rank, C.create_string_buffer(box[0], 128)), "comm_init_rank")
        return cls(h, rank, world)

    @classmethod
    def single(cls):
        """A communicator of one rank on the current device (1-GPU boxes; the exchange degenerates to a copy to self)."""
        buf = C.create_string_buffer(128)
        check(lib().redio_comm_unique_id(buf), "comm_unique_id")
        h = C.c_void_p()
        check(lib().redio_comm_init_rank(C.byref(h), 1, 0, buf), "comm_init_rank")
        return cls(h, 0, 1)

    @classmethod
    def init_all(cls, devices=None):
        """Every visible device (or `devices`) as ranks of ONE process: returns the list of communicators."""
        import torch
        devs = list(range(torch.cuda.device_count())) if devices is None else list(devices)
        hs = (C.c_void_p * len(devs))()
        check(lib().redio_comm_init_all(hs, len(devs), (C.c_int * len(devs))(*devs)), "comm_init_all")
        return [cls(C.c_void_p(hs[i]), i, len(devs)) for i in range(len(devs))]

    def exchange(self, grouped, rows_per_rank, out=None):
        """grouped: [size][my rows][channels per rank] complex64 on this rank's device -> [sum(rows)][channels per rank]."""
        import torch
        assert grouped.dtype == torch.complex64 and grouped.dim() == 3 and grouped.shape[0] == self.size
        rows = [int(r) for r in rows_per_rank]
        assert len(rows) == self.size and rows[self.rank] == grouped.shape[1]
        cpg = grouped.shape[2]
        if out is None:
            out = torch.empty((sum(rows), cpg), dtype=torch.complex64, device=grouped.device)
        check(lib().redio_pfb_exchange(self._h, _dev_ptr(grouped), _dev_ptr(out), (C.c_size_t * self.size)(*rows), cpg, current_stream()),
              "pfb_exchange")
        return out

    def exchange_at(self, grouped, rows_per_rank, out, out_row_offset, stream=None):
        """redio_pfb_exchange_at: rank q's rows land at row out_row_offset[q] of `out`; enqueued on `stream` (a torch stream;
        default: the current one) -- the piece-wise form that overlaps the exchange with the next piece's analysis."""
        rows = [int(r) for r in rows_per_rank]
        offs = [int(o) for o in out_row_offset]
        st = current_stream() if stream is None else C.c_void_p(stream.cuda_stream)
        check(lib().redio_pfb_exchange_at(self._h, _dev_ptr(grouped), _dev_ptr(out), (C.c_size_t * self.size)(*rows),
                                          (C.c_size_t * self.size)(*offs), grouped.shape[2], st), "pfb_exchange_at")
        return out

    def __del__(self, _safe_destroy=_safe_destroy):
        if getattr(self, "_h", None):
            _safe_destroy("redio_comm_destroy", self._h)
            self._h = None


def exchange_all(comms, grouped, rows_per_rank, outs=None):
    """redio_pfb_exchange_all: all ranks of one process (Comm.init_all) in one RCCL group.  grouped[g] lives on device g."""
    import torch
    n = len(comms)
    rows = [int(r) for r in rows_per_rank]
    cpg = grouped[0].shape[2]
    if outs is None:
        outs = [torch.empty((sum(rows), cpg), dtype=torch.complex64, device=grouped[g].device) for g in range(n)]
    streams = [C.c_void_p(torch.cuda.current_stream(grouped[g].device).cuda_stream) for g in range(n)]
    check(lib().redio_pfb_exchange_all((C.c_void_p * n)(*[c._h for c in comms]), n, (C.c_void_p * n)(*[_dev_ptr(t) for t in grouped]),
                                       (C.c_void_p * n)(*[_dev_ptr(t) for t in outs]), (C.c_size_t * n)(*rows), cpg,
                                       (C.c_void_p * n)(*streams)), "pfb_exchange_all")
    return outs


class OverlapSave:
    """redio_ovsave_*: overlap-save FFT convolution (BASELINE.json configs[4]) with the semantics of
    dsputils::convolve (valid-mode correlation, dsputils.rs:30-32) on complex64 streams."""

    def __init__(self, taps, nfft=65536):
        t, p = _taps(taps)
        self.ntaps, self.nfft = len(t), int(nfft)
        self._h = C.c_void_p()
        check(lib().redio_ovsave_create(C.byref(self._h), p, len(t), self.nfft), "ovsave_create")

    def nout(self, n_in):
        return lib().redio_ovsave_nout(self._h, n_in)

    def __call__(self, x, out=None):
        import torch
        assert x.dtype == torch.complex64
        n = self.nout(x.numel())
        if out is None:
            out = torch.empty(n, dtype=torch.complex64, device=x.device)
        check(lib().redio_ovsave_enqueue(self._h, _dev_ptr(x), x.numel(), _dev_ptr(out), current_stream()), "ovsave_enqueue")
        return out[:n]

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_ovsave_destroy", self._h)
            self._h = None


class OverlapSaveReal:
    """redio_ovsave_real_*: overlap-save FFT convolution of a REAL (float32) stream with real taps through kiss_fftr / kiss_fftri, the
    semantics of dsputils::convolve (valid-mode correlation, dsputils.rs:30-32).  An even tap count counts as one more (a zero tap
    behind it): hop = nfft - (ntaps | 1) + 1 is always even.  nfft = 2048 is one kernel (is_fused)."""

    def __init__(self, taps, nfft=2048):
        t, p = _taps(taps)
        self.ntaps, self.nfft = len(t), int(nfft)
        self.hop = self.nfft - (self.ntaps | 1) + 1
        self._h = C.c_void_p()
        check(lib().redio_ovsave_real_create(C.byref(self._h), p, len(t), self.nfft), "ovsave_real_create")

    def nout(self, n_in):
        return lib().redio_ovsave_real_nout(self._h, n_in)

    @property
    def is_fused(self):
        return bool(lib().redio_ovsave_real_is_fused(self._h))

    def reserve(self, n_in):
        check(lib().redio_ovsave_real_reserve(self._h, n_in), "ovsave_real_reserve")

    def __call__(self, x, out=None):
        import torch
        assert x.dtype == torch.float32
        n = self.nout(x.numel())
        if out is None:
            out = torch.empty(n, dtype=torch.float32, device=x.device)
        assert out.dtype == torch.float32 and out.numel() >= n
        check(lib().redio_ovsave_real_enqueue(self._h, _dev_ptr(x), x.numel(), _dev_ptr(out), current_stream()), "ovsave_real_enqueue")
        return out[:n]

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_ovsave_real_destroy", self._h)
            self._h = None


class _PowerSpectrumBase:
    """what PowerSpectrum and PowerSpectrumReal share: a subclass gives its C symbols' prefix, its input dtype and its bins per row"""

    AUTO, ROWS, SEGMENTS = 0, 1, 2
    _prefix = _in_dtype = None

    def _fn(self, name):
        return getattr(lib(), f"redio_{self._prefix}_{name}")

    def __init__(self, bins, nfft, integrate, step, window):
        self.nfft, self.integrate, self._bins = int(nfft), int(integrate), int(bins)
        self.step = self.nfft if step is None else int(step)
        p = None
        if window is not None:
            w, p = _taps(window)
            assert len(w) == self.nfft, "a window of nfft values"
        self._h = C.c_void_p()
        check(self._fn("create")(C.byref(self._h), self.nfft, self.integrate, self.step, p), f"{self._prefix}_create")

    def nrows(self, n_in):
        return self._fn("nrows")(self._h, n_in)

    @property
    def is_fused(self):
        return bool(self._fn("is_fused")(self._h))

    def reserve(self, n_in):
        check(self._fn("reserve")(self._h, n_in), f"{self._prefix}_reserve")

    def set_split(self, mode):
        """AUTO / ROWS (one wavefront per whole row) / SEGMENTS (one per segment of 16 transforms and a fold pass): the same bits."""
        check(self._fn("set_split")(self._h, int(mode)), f"{self._prefix}_set_split")

    def _run(self, name, x, dtype, count, rows, out):
        import torch
        assert x.dtype == getattr(torch, dtype), f"expected torch.{dtype}"
        if out is None:
            out = torch.empty(rows * self._bins, dtype=torch.float32, device=x.device)
        assert out.dtype == torch.float32 and out.numel() >= rows * self._bins
        check(self._fn(name)(self._h, _dev_ptr(x), count, _dev_ptr(out), current_stream()), f"{self._prefix}_{name}")
        return out[: rows * self._bins].view(rows, self._bins)

    def __call__(self, x, out=None):
        return self._run("enqueue", x, self._in_dtype, x.numel(), self.nrows(x.numel()), out)

    def spectra(self, X, out=None):
        """the same integration over packed, already transformed rows of that many bins (a Chain's or an Fftr's output): numel // bins //
        integrate rows"""
        nbatch = X.numel() // self._bins
        return self._run("enqueue_spectra", X, "complex64", nbatch, nbatch // self.integrate, out)

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy(f"redio_{self._prefix}_destroy", self._h)
            self._h = None


class PowerSpectrum(_PowerSpectrumBase):
    """redio_pspec_*: |X[k]|^2 of kissfft::fft blocks (kissfft.rs:18-31) of nfft samples that start every `step` samples, optionally
    windowed, summed over `integrate` consecutive transforms in the blocked order of DESIGN.md 5.3c: complex64 samples in, rows of
    nfft float32 out.  nfft = 1024 is one kernel (is_fused)."""

    _prefix, _in_dtype = "pspec", "complex64"

    def __init__(self, nfft=1024, integrate=1, step=None, window=None):
        super().__init__(nfft, nfft, integrate, step, window)

    def u8(self, raw, out=None):
        """the receiver's interleaved u8 I/Q bytes in (uint8 tensor, even numel): the rows of data_to_samples + __call__, bit for
        bit, without the cf32 intermediate (redio_pspec_enqueue_u8)"""
        assert raw.numel() % 2 == 0, "expected an even number of uint8 bytes"
        return self._run("enqueue_u8", raw, "uint8", raw.numel(), self.nrows(raw.numel() // 2), out)

    def reserve_u8(self, nbytes):
        check(lib().redio_pspec_reserve_u8(self._h, nbytes), "pspec_reserve_u8")


class PowerSpectrumReal(_PowerSpectrumBase):
    """redio_pspec_real_*: |X[k]|^2 of kiss_fftr rows (tools/kiss_fftr.c, the bits of Fftr) of nfft REAL samples that start every
    `step` samples, optionally windowed, summed over `integrate` consecutive transforms in the blocked order of DESIGN.md 5.3c
    (contract: DESIGN.md 5.3d): float32 samples in, rows of nbins = nfft/2 + 1 float32 out.  nfft = 2048 is one kernel (is_fused)."""

    _prefix, _in_dtype = "pspec_real", "float32"

    def __init__(self, nfft=2048, integrate=1, step=None, window=None):
        self.nbins = int(nfft) // 2 + 1
        super().__init__(self.nbins, nfft, integrate, step, window)
        assert lib().redio_pspec_real_nbins(self._h) == self.nbins


class PolyphaseSpectrum:
    """redio_pfb_pspec_*: the polyphase spectrometer -- |row[c]|^2 of a Channelizer's rows (ngroups = 1) summed over `integrate`
    consecutive rows in the blocked order of DESIGN.md 5.3c (contract: DESIGN.md 5.6b), bit for bit Channelizer followed by
    PowerSpectrum(nchan, integrate).spectra: complex64 samples (or, from_bytes, the receiver's u8 I/Q bytes) in, rows of nchan
    float32 out.  64 channels with 4 / 8 / 16 taps per branch are one kernel (is_fused, route WAVE): the channel rows never reach
    memory.  one_kernel=True (REDIO_PFB_PSPEC_BLOCK) asks for the workgroup kernel (route BLOCK) at 32, 128, 256, 512 or 1024
    channels with 4 / 8 / 16 taps per branch, where the channel rows never reach memory either; on every other shape it changes
    nothing.  Every other plan is route GENERIC: the plan's own channelizer into row scratch, then an accumulate pass."""

    AUTO, ROWS, SEGMENTS = 0, 1, 2
    GENERIC, WAVE, BLOCK = 0, 1, 2

    def __init__(self, proto, nchan=64, taps_per_branch=16, integrate=1, fused=True, one_kernel=False):
        t, p = _taps(proto)
        assert len(t) == nchan * taps_per_branch
        self.nchan, self.taps_per_branch, self.integrate = int(nchan), int(taps_per_branch), int(integrate)
        self._h = C.c_void_p()
        flags = (REDIO_FIR_FUSED if fused else 0) | (REDIO_PFB_PSPEC_BLOCK if one_kernel else 0)
        check(lib().redio_pfb_pspec_create(C.byref(self._h), p, self.nchan, self.taps_per_branch, self.integrate, flags), "pfb_pspec_create")

    def nrows(self, n_in):
        return lib().redio_pfb_pspec_nrows(self._h, n_in)

    @property
    def is_fused(self):
        return bool(lib().redio_pfb_pspec_is_fused(self._h))

    @property
    def route(self):
        """what a call runs: GENERIC, WAVE (the 64-channel kernel, is_fused) or BLOCK (the workgroup kernel, one_kernel=True)"""
        return lib().redio_pfb_pspec_route(self._h)

    def reserve(self, n_in, u8=False):
        """all plan scratch (the inner channelizer's included) for calls of up to n_in samples, so that a call never allocates, e.g.
        inside a Graph; u8: for from_bytes calls of as many samples (redio_pfb_pspec_reserve_u8 of twice as many bytes)"""
        if u8:
            check(lib().redio_pfb_pspec_reserve_u8(self._h, 2 * int(n_in)), "pfb_pspec_reserve_u8")
        else:
            check(lib().redio_pfb_pspec_reserve(self._h, int(n_in)), "pfb_pspec_reserve")

    def set_split(self, mode):
        """AUTO / ROWS (a wavefront owns whole output rows) / SEGMENTS (a run of whole 16-row segments, and a fold pass): the same bits."""
        check(lib().redio_pfb_pspec_set_split(self._h, int(mode)), "pfb_pspec_set_split")

    def _run(self, fn, x, count, nsamp, out):
        import torch
        rows = self.nrows(nsamp)
        if out is None:
            out = torch.empty(rows * self.nchan, dtype=torch.float32, device=x.device)
        assert out.dtype == torch.float32 and out.numel() >= rows * self.nchan
        check(getattr(lib(), fn)(self._h, _dev_ptr(x), count, _dev_ptr(out), current_stream()), fn)
        return out[: rows * self.nchan].view(rows, self.nchan)

    def __call__(self, x, out=None):
        import torch
        assert x.dtype == torch.complex64
        return self._run("redio_pfb_pspec_enqueue", x, x.numel(), x.numel(), out)

    def from_bytes(self, raw, out=None):
        """redio_pfb_pspec_enqueue_u8: the rows of bitfount.data_to_samples(raw) followed by this plan, bit for bit"""
        import torch
        assert raw.dtype == torch.uint8 and raw.numel() % 2 == 0
        return self._run("redio_pfb_pspec_enqueue_u8", raw, raw.numel(), raw.numel() // 2, out)

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy("redio_pfb_pspec_destroy", self._h)
            self._h = None


class _TwoPassBankBase:
    """what Synthesizer, OversampledChannelizer and OversampledSynthesizer share: a subclass gives its C symbols' prefix and what a
    call reads and returns"""

    TWO_PASS, WAVE, BLOCK = 0, 1, 2
    _prefix = None

    def _fn(self, name):
        return getattr(lib(), f"redio_{self._prefix}_{name}")

    def _create(self, proto, nchan, taps_per_branch, fused, *hop, more_flags=0):
        t, p = _taps(proto)
        assert len(t) == nchan * taps_per_branch
        self.nchan, self.taps_per_branch = int(nchan), int(taps_per_branch)
        self._h = C.c_void_p()
        check(self._fn("create")(C.byref(self._h), p, self.nchan, self.taps_per_branch, *hop, (REDIO_FIR_FUSED if fused else 0) | more_flags), f"{self._prefix}_create")

    @property
    def route(self):
        """what a call runs: WAVE (the 64-channel kernel; the oversampled plans: at hop 32), BLOCK (the OversampledChannelizer's
        workgroup kernel, one_kernel=True) or TWO_PASS"""
        return self._fn("route")(self._h)

    @property
    def is_fused(self):
        return bool(self._fn("is_fused")(self._h))

    def set_unfused(self, unfused=True):
        """send a WAVE or BLOCK plan down the two-pass route (tests and measurement), or back: the same bits"""
        check(self._fn("set_unfused")(self._h, int(bool(unfused))), f"{self._prefix}_set_unfused")

    def set_chunk_rows(self, rows):
        """rows per pass of the two-pass route (Synthesizer, OversampledSynthesizer: input rows; OversampledChannelizer: rows) (0: the
        64 MiB default); for tests of the chunk seam: the same bits"""
        check(self._fn("set_chunk_rows")(self._h, int(rows)), f"{self._prefix}_set_chunk_rows")

    def reserve(self, n_in):
        """the two-pass route's scratch for calls of up to n_in samples (OversampledChannelizer) or values (Synthesizer,
        OversampledSynthesizer), so that a call never allocates, e.g. inside a Graph"""
        check(self._fn("reserve")(self._h, int(n_in)), f"{self._prefix}_reserve")

    def _run(self, x, n, out, *first_row):
        """enqueue on x into out (allocated here if None) of at least n complex64; returns out"""
        import torch
        assert x.dtype == torch.complex64
        if out is None:
            out = torch.empty(n, dtype=torch.complex64, device=x.device)
        assert out.dtype == torch.complex64 and out.numel() >= n
        check(self._fn("enqueue")(self._h, _dev_ptr(x), x.numel(), *first_row, _dev_ptr(out), current_stream()), f"{self._prefix}_enqueue")
        return out

    def __del__(self, _safe_destroy=_safe_destroy):  # bound at definition: module globals may be gone at shutdown
        if getattr(self, "_h", None):
            _safe_destroy(f"redio_{self._prefix}_destroy", self._h)
            self._h = None


class Synthesizer(_TwoPassBankBase):
    """redio_pfb_synth_*: the synthesis filterbank, many narrow channels into one wideband stream (contract: DESIGN.md 5.6c).  The
    Channelizer is "branch filter, then forward transform"; this is "inverse transform, then the same branch filter": rows of nchan
    complex64 channel values in (the Channelizer's ngroups = 1 layout), kissfft's unnormalised inverse transform per row, then per
    branch the dsputils fold over taps_per_branch rows with g_m[p] = proto[nchan p + m]; (T - taps_per_branch + 1) * nchan samples of
    one stream out.  No 1 / nchan.  64 channels with 4 / 8 / 16 taps per branch are one kernel (route WAVE, is_fused); every other plan
    runs its own inverse transform into scratch and the branch pass (route TWO_PASS): the same bits."""

    _prefix = "pfb_synth"

    def __init__(self, proto, nchan=64, taps_per_branch=16, fused=True):
        self._create(proto, nchan, taps_per_branch, fused)

    def nout(self, n_in):
        return self._fn("nout")(self._h, int(n_in))

    def __call__(self, rows, out=None):
        n = self.nout(rows.numel())
        return self._run(rows, n, out)[:n]


class SynthesizerStream(Stream):
    """redio_pfb_synth_stream_*: a Synthesizer fed as a stream of channel values in messages of ANY length; taps_per_branch - 1 whole
    rows and the values of a partial row are carried, whole output rows come out, and any segmentation concatenates to the one-shot call."""

    def __init__(self, plan):
        assert isinstance(plan, Synthesizer)
        super().__init__(plan)


class OversampledChannelizer(_TwoPassBankBase):
    """redio_pfb_os_*: the oversampled (weighted overlap-add) channelizer, a row of nchan channels every hop <= nchan samples (contract:
    DESIGN.md 5.6d).  The Channelizer's branch filter on the nchan * taps_per_branch samples from r * hop on, the branch sums turned by
    ((first_row + r) * hop) mod nchan places (so that channel k of every row is referred to absolute time), then the forward transform:
    (n_in - nchan * taps_per_branch) // hop + 1 rows of nchan complex64 out.  At hop == nchan these are the Channelizer's rows.  64 channels
    at hop 32 with 4 / 8 / 16 taps per branch are one kernel (route WAVE, is_fused).  one_kernel=True (REDIO_PFB_OS_BLOCK) asks for the
    workgroup kernel (route BLOCK, not is_fused) at 32, 128, 256, 512 or 1024 channels, hop = nchan / 2 and 4 / 8 / 16 taps per branch
    (but 1024 x 16): one launch, no scratch, any 8-byte aligned buffers; on every other shape it changes nothing.  Every other plan runs
    a branch pass into scratch and its own forward transform (route TWO_PASS).  The same bits on all three routes."""

    _prefix = "pfb_os"

    def __init__(self, proto, nchan=64, taps_per_branch=16, hop=32, fused=True, one_kernel=False):
        self._create(proto, nchan, taps_per_branch, fused, int(hop), more_flags=REDIO_PFB_OS_BLOCK if one_kernel else 0)

    @property
    def hop(self):
        return self._fn("hop")(self._h)

    def nrows(self, n_in):
        return self._fn("nrows")(self._h, int(n_in))

    def __call__(self, x, first_row=0, out=None):
        rows = self.nrows(x.numel())
        return self._run(x, rows * self.nchan, out, int(first_row)).reshape(-1)[: rows * self.nchan].reshape(rows, self.nchan)


class OversampledChannelizerStream(Stream):
    """redio_pfb_os_stream_*: an OversampledChannelizer fed as a stream in messages of ANY length; the samples from the next row's first
    one on and the running row index are carried, whole rows come out (flat), and any segmentation concatenates to the one-shot call
    with first_row = 0."""

    def __init__(self, plan):
        assert isinstance(plan, OversampledChannelizer)
        super().__init__(plan)


class OversampledSynthesizer(_TwoPassBankBase):
    """redio_pfb_os_synth_*: the oversampled synthesis bank, the OversampledChannelizer's rows back into one stream (contract: DESIGN.md
    5.6e).  kissfft's unnormalised inverse transform of every row of nchan channel values, then a weighted overlap-add at hop <= nchan:
    with L = ceil(nchan * taps_per_branch / hop), T rows in give (T - L + 1) * hop complex64 samples, sample n at absolute time
    (first_row + L - 1) * hop + n.  At hop == nchan this is the Synthesizer.  64 channels at hop 32 with 4 / 8 / 16 taps per branch are
    one kernel (route WAVE, is_fused); every other plan runs its own inverse transform into scratch and an overlap-add pass (route
    TWO_PASS): the same bits."""

    _prefix = "pfb_os_synth"

    def __init__(self, proto, nchan=64, taps_per_branch=16, hop=32, fused=True):
        self._create(proto, nchan, taps_per_branch, fused, int(hop))

    @property
    def hop(self):
        return self._fn("hop")(self._h)

    def nout(self, n_in):
        return self._fn("nout")(self._h, int(n_in))

    def __call__(self, x, first_row=0, out=None):
        n = self.nout(x.numel())
        return self._run(x, n, out, int(first_row)).reshape(-1)[:n]


class OversampledSynthesizerStream(Stream):
    """redio_pfb_os_synth_stream_*: an OversampledSynthesizer fed as a stream of channel values in messages of ANY length; L - 1 whole rows,
    the values of a partial row and the running row index are carried, whole hops of samples come out, and any segmentation
    concatenates to the one-shot call with first_row = 0."""

    def __init__(self, plan):
        assert isinstance(plan, OversampledSynthesizer)
        super().__init__(plan)
