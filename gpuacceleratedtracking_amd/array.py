"""Antenna-array processing on device tensors (include/gat.h, "antenna-array processing"): the spatial covariance of the raw
samples, beamformer weights from it, and the weights applied to correlator accumulators or to the raw samples.

Correlation is linear, so a beam or a null is applied to the accumulators the correlators already return:
``w^H (sum_n x_n c_n) = sum_n (w^H x_n) c_n``.  A receiver estimates ``R = spatial_covariance(signal, N, B)``, turns it into
``w = beamformer_weights(R, steering)`` and hands ``w`` to ``TrackingLoop(weights=w)`` (or to ``beamform`` for accumulators
it already has).  ``beamform_samples`` applies the weights before correlation instead, ``y[n] = w^H x[n]``: the beam is a
signal of its own, which is what the acquisition search needs under a jammer (``acquire(..., weights=w)``).  Everything runs in libgat's HIP kernels; there is no CPU fallback."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from ._lib import GAT_BF_CONVENTIONAL, GAT_BF_MVDR, GAT_BF_POWER_INVERSION  # noqa: F401
from .context import Context, get_context
from .streams import alloc_stream, input_desc, keep_alive, planes, vp

_planes = planes  # the name the tests reach for
_MODES = {"conventional": GAT_BF_CONVENTIONAL, "mvdr": GAT_BF_MVDR, "power_inversion": GAT_BF_POWER_INVERSION}


def spatial_covariance(signal, num_samples: int, num_blocks: int = 1, blocks_per_estimate: int | None = None, start: int = 0,
                       block_stride: int | None = None, ctx: Context | None = None) -> torch.Tensor:
    """``R_e[i, j] = sum_{b in e} sum_{n < N} x[n, i, b] conj(x[n, j, b])`` (a plain sum) as complex64 ``[E, M, M]``, with
    ``E = ceil(num_blocks / blocks_per_estimate)`` (default: one estimate over all blocks).  ``signal`` and its blocks as
    ``streams.input_desc`` takes them.  Exactly Hermitian, and the same bits on every call."""
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    nb = int(num_blocks)
    bpe = nb if blocks_per_estimate is None else int(blocks_per_estimate)
    if bpe < 1:
        raise ValueError("blocks_per_estimate must be positive")
    ctx = ctx if ctx is not None else get_context(re.device)
    E, M = (nb + bpe - 1) // bpe, int(desc.num_ants)
    cov_re = torch.empty((E, M, M), dtype=torch.float32, device=re.device)
    cov_im = torch.empty_like(cov_re)
    ctx.check(ctx.lib.gat_spatial_covariance(ctx._h, C.byref(desc), nb, bpe, vp(cov_re), vp(cov_im)), "gat_spatial_covariance")
    return torch.complex(cov_re, cov_im)


def beamformer_weights(cov: torch.Tensor | None, steering: torch.Tensor | None = None, mode="mvdr", loading: float = 0.0,
                       ctx: Context | None = None) -> torch.Tensor:
    """Weights complex128 ``[K, M]`` on the device from one covariance ``cov`` (complex ``[M, M]``, e.g. one estimate of
    ``spatial_covariance``) and ``steering`` (complex ``[K, M]`` or ``[M]``): ``"conventional"`` a / (a^H a), ``"mvdr"``
    R'^-1 a / (a^H R'^-1 a), ``"power_inversion"`` R'^-1 e0 / (e0^H R'^-1 e0) (no steering vector; one row), with
    R' = R + loading * trace(R) / M * I.  FP64 Cholesky on the device; a covariance that is not positive definite gives NaN
    weights."""
    m = _MODES[mode] if isinstance(mode, str) else int(mode)
    ref = cov if cov is not None else steering
    if ref is None:
        raise ValueError("neither a covariance nor a steering vector")
    dev = ref.device
    ctx = ctx if ctx is not None else get_context(dev)
    a_re = a_im = None
    K = 1
    if steering is not None:
        st = steering.reshape(1, -1) if steering.dim() == 1 else steering
        a_re, a_im = planes(st.to(dev), torch.float64)
        K = int(st.shape[0])
    c_re = c_im = None
    if cov is not None:
        if cov.dim() != 2 or cov.shape[0] != cov.shape[1]:
            raise ValueError("cov must be [M, M] (pick one estimate of spatial_covariance)")
        c_re, c_im = planes(cov, torch.float32)
    M = int(cov.shape[0] if cov is not None else a_re.shape[1])
    if a_re is not None and a_re.shape[1] != M:
        raise ValueError("steering and covariance disagree on the number of antennas")
    w_re = torch.empty((K, M), dtype=torch.float64, device=dev)
    w_im = torch.empty_like(w_re)
    ctx.check(ctx.lib.gat_array_weights(ctx._h, vp(c_re), vp(c_im), M, vp(a_re), vp(a_im), K, m, float(loading), vp(w_re), vp(w_im)),
              "gat_array_weights")
    return keep_alive(torch.complex(w_re, w_im), c_re, c_im, a_re, a_im)


def beamform(acc_re: torch.Tensor, acc_im: torch.Tensor, weights: torch.Tensor, ctx: Context | None = None):
    """``y[b, k, l] = sum_m conj(w[k, m]) acc[b, k, l, m]``: float32 accumulators ``[B, K, L, M]`` (or ``[K, L, M]``) as the
    correlators write them, ``weights`` complex ``[K, M]``.  Returns ``(y_re, y_im)`` float32 without the antenna axis."""
    if acc_re.shape != acc_im.shape or acc_re.dtype != torch.float32 or acc_im.dtype != torch.float32:
        raise ValueError("accumulator planes must be float32 of one shape")
    shape = acc_re.shape
    if len(shape) not in (3, 4):
        raise ValueError("accumulators must be [B, K, L, M] or [K, L, M]")
    B = int(shape[0]) if len(shape) == 4 else 1
    K, L, M = (int(x) for x in shape[-3:])
    if tuple(weights.shape) != (K, M):
        raise ValueError("weights must be [K, M]")
    ctx = ctx if ctx is not None else get_context(acc_re.device)
    w_re, w_im = planes(weights.to(acc_re.device), torch.float64)
    a_re, a_im = acc_re.contiguous(), acc_im.contiguous()
    y_re = torch.empty(shape[:-1], dtype=torch.float32, device=acc_re.device)
    y_im = torch.empty_like(y_re)
    ctx.check(ctx.lib.gat_beamform(ctx._h, vp(a_re), vp(a_im), B, K, L, M, vp(w_re), vp(w_im), vp(y_re), vp(y_im)), "gat_beamform")
    return keep_alive((y_re, y_im), w_re, w_im, a_re, a_im)


def beamform_desc(ctx: Context, desc: _lib.SignalDesc, weights: torch.Tensor, num_blocks: int, out_block_stride: int | None = None,
                  interleaved: bool = False, zero: bool = True):
    """``gat_beamform_samples`` of the ``num_blocks`` blocks a signal descriptor covers.  Returns ``(out, out_desc)``: the
    tensors ``beamform_samples`` returns, and the descriptor of them as a J-antenna signal (it points into ``out``: keep both).
    ``zero=False`` leaves what the kernel does not write uninitialised (no gaps to fill when blocks are back to back)."""
    N, M, nb = int(desc.num_samples), int(desc.num_ants), int(num_blocks)
    w = weights.reshape(1, -1) if weights.dim() == 1 else weights
    if w.dim() != 2 or int(w.shape[1]) != M:
        raise ValueError("weights must be [J, M] or [M]")
    J = int(w.shape[0])
    out, odesc = alloc_stream(J, N, nb, ctx.device, planar=not interleaved, block_stride=N if out_block_stride is None else out_block_stride,
                              zero=zero)  # (the documented default is unpadded: blocks back to back)
    w_re, w_im = planes(w.to(ctx.device), torch.float64)
    ctx.check(ctx.lib.gat_beamform_samples(ctx._h, C.byref(desc), nb, vp(w_re), vp(w_im), J, C.byref(odesc)), "gat_beamform_samples")
    return out, keep_alive(odesc, w_re, w_im)


def beamform_samples(signal, weights: torch.Tensor, num_samples: int, num_blocks: int = 1, start: int = 0, block_stride: int | None = None,
                     out_block_stride: int | None = None, interleaved: bool = False, ctx: Context | None = None):
    """Beams of the raw samples, ``y[j, n] = sum_m conj(w[j, m]) x[m, n]`` for every sample of ``num_blocks`` blocks.
    ``signal`` as ``streams.input_desc`` takes it; ``weights`` complex (or real) ``[J, M]`` or ``[M]`` of any float dtype,
    moved to the float64 planes ``beamformer_weights`` returns.  Returns ``(re, im)`` float32 ``[J, num_blocks *
    out_block_stride]``, or with ``interleaved=True`` one tensor ``[J, num_blocks * out_block_stride, 2]``; block b starts
    ``b * out_block_stride`` samples in (default: ``num_samples``; what a larger stride leaves between blocks is zero: the
    allocation's, the kernel does not write there).  The result is a J-antenna signal for ``acquire``, ``spatial_covariance``
    and the correlators.  float32 sums in antenna order: ``|y - y64| <= (4 M + 4) 2^-24 sum_m |w_m| |x_m|``."""
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    ctx = ctx if ctx is not None else get_context(re.device)
    out, odesc = beamform_desc(ctx, desc, weights, int(num_blocks), out_block_stride, interleaved)
    return keep_alive(out, odesc)  # (the descriptor holds the weights)
