"""Sample filtering on device tensors (include/gat.h, "sample filtering"): a complex FIR with decimation and a numerically
controlled oscillator over the raw samples -- stream in, stream out -- and the tap design that goes with it.

A notch against a CW tone, at the stream's own rate::

    y, desc = filter_samples((re, im), notch_taps(33, nu, 0.01), N, num_blocks=B)
    results = acquire(system, desc, fs, prns, num_blocks=B)

and a channeliser from a wideband front end down to the rate the search and the correlators are fast at::

    y, desc, fs_out, delay = channelize(x, 100e6, 12.5e6, 8e6, 5, 64, total_samples=n)

Everything runs in libgat's HIP kernels; there is no CPU fallback (``filter_samples_host`` is the library's host twin, the
bit-exact reference of the device call, for tests and for machines without a GPU).  Taps are designed in numpy float64 and
narrowed to float32 once."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .streams import addr, alloc_stream, input_desc, keep_alive, output_desc, overlap_save_blocks, ref, stream_views, vp
from .streams import host_desc  # noqa: F401  (the name the host twin's docstring points to)


# ---- tap design (numpy float64) ------------------------------------------------------------------------------------------------
def lowpass_taps(num_taps: int, cutoff: float, window: str = "kaiser", beta: float = 8.0) -> np.ndarray:
    """Windowed-sinc low-pass, float64 ``[num_taps]``, unit gain at DC; ``cutoff`` in cycles/sample (the -6 dB point, below 0.5).
    ``window``: "kaiser" (``beta`` 8: about 80 dB of stop band, transition width about 5 / num_taps), "hamming", "hann",
    "blackman" or "rect"."""
    T = int(num_taps)
    if T < 1 or not 0.0 < float(cutoff) <= 0.5:
        raise ValueError("num_taps must be positive and 0 < cutoff <= 0.5 cycles/sample")
    n = np.arange(T, dtype=np.float64) - (T - 1) / 2.0
    h = 2.0 * cutoff * np.sinc(2.0 * cutoff * n)
    wins = {"kaiser": lambda: np.kaiser(T, beta), "hamming": lambda: np.hamming(T), "hann": lambda: np.hanning(T),
            "blackman": lambda: np.blackman(T), "rect": lambda: np.ones(T)}
    if window not in wins:
        raise ValueError(f"unknown window {window!r}")
    h = h * wins[window]()
    return h / h.sum()


def shift_taps(taps, nu: float) -> np.ndarray:
    """``h[t] * exp(+j 2 pi nu t)``, complex128: the filter whose pass band sits at ``nu`` cycles/sample.  With ``nco_step = nu``
    it is "mix down by nu, then filter with h"."""
    h = np.asarray(taps)
    return h.astype(np.complex128) * np.exp(2j * np.pi * float(nu) * np.arange(h.size, dtype=np.float64))


def notch_taps(num_taps: int, nu: float, width: float, window: str = "kaiser", beta: float = 8.0) -> np.ndarray:
    """A delta at the centre tap minus a low-pass of cutoff ``width`` shifted to ``nu`` (cycles/sample), complex128: a null at ``nu``
    (the shifted low-pass has gain exp(j 2 pi nu c) there, the delayed delta too), unit gain away from it, a group delay of
    ``c = (num_taps - 1) / 2`` samples.  ``num_taps`` must be odd."""
    T = int(num_taps)
    if T % 2 == 0:
        raise ValueError("a notch needs an odd number of taps (a centre tap)")
    c = (T - 1) // 2
    g = -shift_taps(lowpass_taps(T, width, window, beta), nu) * np.exp(-2j * np.pi * float(nu) * c)
    g[c] += 1.0
    return g


def _tap_planes(taps):
    g = np.asarray(taps)
    if g.ndim != 1 or g.size < 1:
        raise ValueError("taps must be a one-dimensional array")
    g = g.astype(np.complex128)
    return np.ascontiguousarray(g.real, dtype=np.float32), np.ascontiguousarray(g.imag, dtype=np.float32)


def _config(T: int, decimation: int, nco_step: float, nco_phase: float) -> _lib.FirConfig:
    return _lib.FirConfig(C.sizeof(_lib.FirConfig), int(T), int(decimation), float(nco_step), float(nco_phase))


def num_outputs(num_samples: int, num_taps: int, decimation: int = 1) -> int:
    """``Q = (N - T) / D + 1``: the outputs of a block of ``num_samples``"""
    return (int(num_samples) - int(num_taps)) // int(decimation) + 1


def _alloc_out(M: int, Q: int, nb: int, interleaved: bool, device):
    """``alloc_stream`` for a float32 output, in the argument order the tests call it with."""
    return alloc_stream(M, Q, nb, device, planar=not interleaved)


def filter_samples(signal, taps, num_samples: int, num_blocks: int = 1, decimation: int = 1, nco_step: float = 0.0, nco_phase: float = 0.0,
                   start: int = 0, block_stride: int | None = None, interleaved: bool = False, out=None, ctx: Context | None = None,
                   out_block_stride: int | None = None):
    """``y[q] = exp(-j 2 pi (P step + phase)) sum_t taps[t] x[q D + T - 1 - t]`` for every block of ``num_samples`` input samples
    (``P``: the newest sample's position in the stream, ``start`` excluded), ``Q = (num_samples - T) / D + 1`` outputs a block.
    ``signal`` as ``streams.input_desc`` takes it (any of the four layouts); ``taps`` real or complex ``[T]``, narrowed to float32.
    Returns ``(tensor(s), desc)``: a float32 ``(re, im)`` pair ``[M, Ntot]`` or, with ``interleaved=True``, one tensor ``[M, Ntot,
    2]``, and its descriptor (it points into the tensor: keep both), which ``acquire``, ``spatial_covariance``,
    ``beamform_samples``, ``sample_stats`` / ``condition_samples`` and the correlators take as it is.  Allocated here, block b
    starts ``b * stride`` outputs in with ``stride`` = Q rounded up to 16 bytes (what lies between blocks is zero); a caller's
    ``out`` (with ``out_block_stride``, default Q) is described as it is."""
    g_re, g_im = _tap_planes(taps)
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    nb, N, M, T, D = int(num_blocks), int(num_samples), int(desc.num_ants), g_re.size, int(decimation)
    if D < 1 or N < T:
        raise ValueError("decimation must be positive and a block no shorter than the filter")
    Q = num_outputs(N, T, D)
    ctx = ctx if ctx is not None else get_context(re.device)
    t_re, t_im = torch.from_numpy(g_re).to(re.device), torch.from_numpy(g_im).to(re.device)
    if out is None:
        out, odesc = alloc_stream(M, Q, nb, re.device, planar=not interleaved)
    else:
        odesc = output_desc(out, Q, out_block_stride)
    cfg = _config(T, D, nco_step, nco_phase)
    ctx.check(ctx.lib.gat_filter_samples(ctx._h, C.byref(desc), nb, vp(t_re), vp(t_im), C.byref(cfg), C.byref(odesc)), "gat_filter_samples")
    return out, keep_alive(odesc, t_re, t_im)


def filter_samples_host(desc: _lib.SignalDesc, num_blocks: int, taps, out_desc: _lib.SignalDesc, decimation: int = 1, nco_step: float = 0.0,
                        nco_phase: float = 0.0, config: _lib.FirConfig | None = None) -> int:
    """``gat_filter_samples_host`` on descriptors of HOST memory (``host_desc`` builds one over numpy arrays).  Returns the status
    instead of raising: the refusals are part of what the twin is a reference of.  ``taps``: real or complex ``[T]``, a pair of
    float32 planes (either may be None: a null pointer), or None; ``config`` overrides the one made of the other arguments."""
    if taps is None:
        g_re = g_im = None
    elif isinstance(taps, tuple):
        g_re, g_im = taps
    else:
        g_re, g_im = _tap_planes(taps)
    T = g_re.size if g_re is not None else (g_im.size if g_im is not None else 1)
    cfg = config if config is not None else _config(T, decimation, nco_step, nco_phase)
    return int(_lib.load().gat_filter_samples_host(ref(desc), int(num_blocks), addr(g_re), addr(g_im), C.byref(cfg), ref(out_desc)))


def stream_blocks(total_samples: int, num_taps: int, decimation: int, num_blocks: int = 1):
    """Overlap-save geometry of a contiguous stream of ``total_samples``: ``(N, in_stride, Q, B, outputs)`` -- B blocks of N = Q D +
    T - 1 input samples every Q D samples give Q outputs each, ``outputs = B Q`` in all (the stream's own (total - T) / D + 1,
    rounded down to a multiple of B)."""
    if int(num_blocks) < 1 or int(total_samples) < int(num_taps):
        raise ValueError("num_blocks must be positive and the stream no shorter than the filter")
    return overlap_save_blocks(total_samples, num_taps, decimation, num_blocks)


def filter_stream(signal, taps, total_samples: int, decimation: int = 1, nco_step: float = 0.0, nco_phase: float = 0.0, num_blocks: int = 1,
                  start: int = 0, interleaved: bool = False, ctx: Context | None = None):
    """One contiguous stream of ``total_samples`` through the filter as ``num_blocks`` overlapping blocks (overlap-save by
    descriptor: no carry state), written back to back: ONE seamless output of ``num_blocks * Q`` samples whose bits do not depend
    on ``num_blocks``.  Returns ``(tensor(s), desc)``; the descriptor is one block of all the outputs."""
    g_re, _ = _tap_planes(taps)
    N, stride, Q, B, total_out = stream_blocks(total_samples, g_re.size, decimation, num_blocks)
    re, desc = input_desc(signal, N, B, start, stride)
    M = int(desc.num_ants)
    out = stream_views(alloc_stream(M, total_out, 1, re.device, planar=not interleaved)[0], total_out)
    _, odesc = filter_samples(signal, taps, N, B, decimation, nco_step, nco_phase, start, stride, interleaved, out, ctx, out_block_stride=Q)
    odesc.num_samples, odesc.block_stride = total_out, total_out
    return out, odesc


def channelize(signal, fs: float, center_hz: float, cutoff_hz: float, decimation: int, num_taps: int, total_samples: int | None = None,
               num_blocks: int = 1, window: str = "kaiser", beta: float = 8.0, nco_phase: float = 0.0, start: int = 0, interleaved: bool = False,
               ctx: Context | None = None):
    """The band around ``center_hz`` of a stream sampled at ``fs``, brought to baseband, low-passed at ``cutoff_hz`` and decimated:
    ``shift_taps(lowpass_taps(num_taps, cutoff_hz / fs), center_hz / fs)`` with ``nco_step = center_hz / fs``, through
    ``filter_stream``.  Returns ``(tensor(s), desc, fs / decimation, delay)`` with ``delay`` the filter's group delay in OUTPUT
    samples: output q shows the input at sample ``q * decimation + (num_taps - 1) / 2``, so an event at input time t appears at
    output sample ``t * fs / decimation - delay``."""
    re = signal[0] if isinstance(signal, (tuple, list)) else signal
    if total_samples is None:
        total_samples = (re.shape[-1] if isinstance(signal, (tuple, list)) else re.shape[-2]) - int(start)
    nu = float(center_hz) / float(fs)
    taps = shift_taps(lowpass_taps(num_taps, float(cutoff_hz) / float(fs), window, beta), nu)
    out, desc = filter_stream(signal, taps, total_samples, decimation, nu, nco_phase, num_blocks, start, interleaved, ctx)
    return out, desc, float(fs) / int(decimation), (int(num_taps) - 1) / 2.0 / int(decimation)
