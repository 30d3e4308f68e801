"""Sample conditioning on device tensors (include/gat.h, "sample conditioning"): level statistics per antenna with pulses
excluded, the AGC's records from them, and the conditioned stream -- blanked, scaled, requantised -- that ``acquire``,
``spatial_covariance``, ``beamform_samples`` and the correlators take as a signal.

The fastest kernels read int8 pairs; ``requantize`` is what makes them from a float front end::

    sig8, desc, counts, params = requantize((re, im), N, num_blocks=B, blank_factor=4.0)
    results = acquire(sig8, system, fs, N, prns, ...)

Everything runs in libgat's HIP kernels; there is no CPU fallback (``condition_samples_host`` and ``agc_params_host`` are the
library's host twins, the bit-exact reference of the device calls, for tests and for machines without a GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import COND_PARAMS_DTYPE, GAT_COND_BLANK_ALL_ANTS, SAMPLE_STATS_DTYPE  # noqa: F401
from .context import Context, get_context
from .results import host_check
from .streams import addr, alloc_stream, input_desc, keep_alive, output_desc, ref, vp
from .streams import host_desc  # noqa: F401  (the name the host twins' docstrings point to)


class SampleStats:
    """``gat_sample_stats_t`` records ``[E, M]`` on the device: ``raw`` is the uint8 tensor ``[E, M, 48]`` the kernel wrote;
    ``numpy()`` copies it to the host as a structured array (kept, blanked, sum_re, sum_im, sum_pow, max_abs); ``stats[e]`` is
    one estimate (a view)."""

    def __init__(self, raw: torch.Tensor):
        self.raw = raw

    @property
    def shape(self):
        return tuple(self.raw.shape[:2])

    def __getitem__(self, e: int) -> "SampleStats":
        E = self.raw.shape[0]
        if not -E <= e < E:
            raise IndexError(f"estimate {e} of {E}")
        e %= E
        return SampleStats(self.raw[e:e + 1])

    def numpy(self) -> np.ndarray:
        return self.raw.cpu().numpy().view(SAMPLE_STATS_DTYPE).reshape(self.shape)


def _records(params, M: int, device) -> torch.Tensor:
    """``gat_cond_params`` records as a float32 tensor ``[M, 4]`` (scale, dc_re, dc_im, threshold) on ``device``."""
    if isinstance(params, np.ndarray):
        params = torch.from_numpy(np.ascontiguousarray(params).view(np.float32).reshape(-1, 4).copy())
    t = params.to(device=device, dtype=torch.float32).contiguous()
    if tuple(t.shape) != (M, 4):
        raise ValueError(f"params must be [M, 4] = (scale, dc_re, dc_im, threshold) for {M} antennas")
    return t


def sample_stats(signal, num_samples: int, num_blocks: int = 1, blocks_per_estimate: int | None = None, params=None,
                 blank_all: bool = False, ctx: Context | None = None, start: int = 0, block_stride: int | None = None,
                 out: SampleStats | None = None) -> SampleStats:
    """Level statistics per (estimate, antenna) over the samples the blanking rule keeps: counts, ``sum x``, ``sum |x|^2`` and
    the largest component, ``E = ceil(num_blocks / blocks_per_estimate)`` estimates (default: one over all blocks).  ``signal``
    as ``streams.input_desc`` takes it.  ``params``: records ``[M, 4]`` of which only the threshold is read, or None (keep every
    sample).  The same bits on every call; FP64 sums.  ``out``: an earlier result to write into (no allocation)."""
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    nb = int(num_blocks)
    bpe = nb if blocks_per_estimate is None else int(blocks_per_estimate)
    if bpe < 1:
        raise ValueError("blocks_per_estimate must be positive")
    ctx = ctx if ctx is not None else get_context(re.device)
    E, M = (nb + bpe - 1) // bpe, int(desc.num_ants)
    prm = _records(params, M, re.device) if params is not None else None
    if out is None:
        out = SampleStats(torch.empty((E, M, SAMPLE_STATS_DTYPE.itemsize), dtype=torch.uint8, device=re.device))
    elif out.shape != (E, M):
        raise ValueError("out has another shape")
    flags = GAT_COND_BLANK_ALL_ANTS if blank_all else 0
    ctx.check(ctx.lib.gat_sample_stats(ctx._h, C.byref(desc), nb, bpe, vp(prm), flags, vp(out.raw)), "gat_sample_stats")
    return keep_alive(out, prm)


def _agc_config(target_rms: float, blank_factor: float, remove_dc: bool) -> _lib.AgcConfig:
    return _lib.AgcConfig(C.sizeof(_lib.AgcConfig), float(target_rms), float(blank_factor), int(bool(remove_dc)))


def agc_params(stats: SampleStats, target_rms: float, blank_factor: float = 0.0, remove_dc: bool = False, ctx: Context | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """The next records ``[M, 4]`` (scale, dc_re, dc_im, threshold; float32, on the device) from ONE estimate's statistics,
    without a host round trip: ``sigma = sqrt(sum_pow / (2 kept))``, ``scale = target_rms / sigma``, ``dc = sum / kept`` if
    ``remove_dc``, ``threshold = blank_factor * sigma`` (``blank_factor <= 0``: no blanking).  An antenna without kept samples
    or power gets scale 0 and no blanking."""
    E, M = stats.shape
    if E != 1:
        raise ValueError("pick one estimate: stats[e]")
    ctx = ctx if ctx is not None else get_context(stats.raw.device)
    if out is None:
        out = torch.empty((M, 4), dtype=torch.float32, device=stats.raw.device)
    elif tuple(out.shape) != (M, 4) or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("out must be a contiguous float32 [M, 4]")
    cfg = _agc_config(target_rms, blank_factor, remove_dc)
    ctx.check(ctx.lib.gat_agc_update(ctx._h, vp(stats.raw), M, C.byref(cfg), vp(out)), "gat_agc_update")
    return out


def agc_params_host(stats: np.ndarray, target_rms: float, blank_factor: float = 0.0, remove_dc: bool = False) -> np.ndarray:
    """``gat_agc_update_host``: the same arithmetic on a host structured array ``[M]`` of ``SAMPLE_STATS_DTYPE``."""
    st = np.ascontiguousarray(stats, dtype=SAMPLE_STATS_DTYPE).reshape(-1)
    out = np.zeros(st.size, dtype=COND_PARAMS_DTYPE)
    cfg = _agc_config(target_rms, blank_factor, remove_dc)
    rc = _lib.load().gat_agc_update_host(addr(st), st.size, C.byref(cfg), addr(out))
    host_check(rc, "gat_agc_update_host")
    return out


def condition_samples(signal, params, num_samples: int, num_blocks: int = 1, out_dtype=torch.int8, blank_all: bool = False, out=None,
                      ctx: Context | None = None, start: int = 0, block_stride: int | None = None, planar: bool = False,
                      out_block_stride: int | None = None, counts: torch.Tensor | None = None):
    """The conditioned stream: a sample of antenna m is blanked unless ``|re| <= T_m and |im| <= T_m`` (``blank_all``: on every
    antenna if on any), a kept component becomes ``(x - dc) * scale`` in float32 and, for an integer ``out_dtype``, is rounded
    to nearest-even and clamped to +-127 / +-32767.  Returns ``(tensor, desc, counts)``: the output as ``acquire`` and the
    correlators take it -- ``[M, Ntot, 2]`` of ``out_dtype``, or with ``planar=True`` a float32 ``(re, im)`` pair ``[M, Ntot]`` --,
    its descriptor (it points into the tensor: keep both) and int64 ``[M, 2]`` = (blanked samples, clipped components), added
    to ``counts`` when one is passed.  Allocated here, block b starts ``b * stride`` samples in with ``stride`` = ``num_samples``
    rounded up to 16 bytes (what lies between blocks is zero); a caller's ``out`` (with ``out_block_stride``, default
    ``num_samples``) is described as it is -- the input itself for in-place work."""
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    nb, N, M = int(num_blocks), int(num_samples), int(desc.num_ants)
    ctx = ctx if ctx is not None else get_context(re.device)
    prm = _records(params, M, re.device)
    if out is None:
        out, odesc = alloc_stream(M, N, nb, re.device, out_dtype, planar)
    else:
        odesc = output_desc(out, N, out_block_stride)
    if counts is None:
        counts = torch.zeros((M, 2), dtype=torch.int64, device=re.device)
    flags = GAT_COND_BLANK_ALL_ANTS if blank_all else 0
    ctx.check(ctx.lib.gat_condition_samples(ctx._h, C.byref(desc), nb, vp(prm), flags, C.byref(odesc), vp(counts)), "gat_condition_samples")
    return out, keep_alive(odesc, prm), counts


def condition_samples_host(desc: _lib.SignalDesc, num_blocks: int, params: np.ndarray, out_desc: _lib.SignalDesc, blank_all: bool = False,
                           counts: np.ndarray | None = None) -> int:
    """``gat_condition_samples_host`` on descriptors of HOST memory (``host_desc`` builds one over numpy arrays).  Returns the
    status instead of raising: the refusals are part of what the twin is a reference of."""
    prm = np.ascontiguousarray(params, dtype=COND_PARAMS_DTYPE) if params is not None else None
    if counts is not None and (counts.dtype != np.uint64 or not counts.flags.c_contiguous):
        raise ValueError("counts must be a contiguous uint64 [M, 2]")
    flags = GAT_COND_BLANK_ALL_ANTS if blank_all is True else int(blank_all)
    return int(_lib.load().gat_condition_samples_host(ref(desc), int(num_blocks), addr(prm), flags, ref(out_desc), addr(counts)))


def requantize(signal, num_samples: int, num_blocks: int = 1, out_dtype=torch.int8, target_rms: float = 16.0, blank_factor: float = 0.0,
               iterations: int = 2, remove_dc: bool = False, blank_all: bool = False, ctx: Context | None = None, start: int = 0,
               block_stride: int | None = None, planar: bool = False):
    """Measure, set the gain, convert: ``iterations`` rounds of ``sample_stats`` (one estimate over all blocks, blanking with
    the previous round's threshold) and ``agc_params``, then ``condition_samples``.  Two rounds are the robust iteration: a
    pulse inflates the first sigma, the second measurement excludes it.  Returns ``(tensor, desc, counts, params)``.

    The default ``target_rms = 16`` counts per component for int8: the clip at 127 is 127 / 16 = 7.9 sigma away (a Gaussian
    component passes it with probability 2e-15), and the quantisation step is sigma / 16, which adds 1 / (12 * 256) = 0.03 % to
    the noise power (0.0014 dB).  For int16 a larger target costs nothing."""
    if int(iterations) < 1:
        raise ValueError("iterations must be at least 1")
    params = None
    for _ in range(int(iterations)):
        st = sample_stats(signal, num_samples, num_blocks, None, params, blank_all, ctx, start, block_stride)
        params = agc_params(st, target_rms, blank_factor, remove_dc, ctx)
    out, desc, counts = condition_samples(signal, params, num_samples, num_blocks, out_dtype, blank_all, None, ctx, start, block_stride, planar)
    return out, desc, counts, params
