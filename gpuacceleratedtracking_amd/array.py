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
from .tracking import _signal_desc

_MODES = {"conventional": GAT_BF_CONVENTIONAL, "mvdr": GAT_BF_MVDR, "power_inversion": GAT_BF_POWER_INVERSION}


def _vp(t: torch.Tensor | None):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def spatial_covariance(signal, num_samples: int, num_blocks: int = 1, blocks_per_estimate: int | None = None, start: int = 0,
                       block_stride: int | None = None, ctx: Context | None = None) -> torch.Tensor:
    """``R_e[i, j] = sum_{b in e} sum_{n < N} x[n, i, b] conj(x[n, j, b])`` (a plain sum) as complex64 ``[E, M, M]``, with
    ``E = ceil(num_blocks / blocks_per_estimate)`` (default: one estimate over all blocks).  ``signal``: a planar pair
    ``(re, im)`` of float32 ``[M, Ntot]`` or one interleaved tensor ``[M, Ntot, 2]`` of float32 / int16 / int8; block b
    starts ``start + b * block_stride`` samples in (default stride: ``num_samples``).  Exactly Hermitian, and the same bits
    on every call."""
    re, im = signal if isinstance(signal, (tuple, list)) else (signal, None)
    nb = int(num_blocks)
    bpe = nb if blocks_per_estimate is None else int(blocks_per_estimate)
    if nb < 1 or bpe < 1:
        raise ValueError("num_blocks and blocks_per_estimate must be positive")
    stride = int(num_samples) if block_stride is None else int(block_stride)
    ntot = re.shape[-2] if im is None else re.shape[-1]
    if stride < 0 or start + (nb - 1) * stride + num_samples > ntot:
        raise ValueError("signal shorter than start + (num_blocks - 1) * block_stride + num_samples")
    ctx = ctx if ctx is not None else get_context(re.device)
    desc = _signal_desc(re, im, int(num_samples), start=int(start), block_stride=stride)
    E, M = (nb + bpe - 1) // bpe, int(desc.num_ants)
    cov_re = torch.empty((E, M, M), dtype=torch.float32, device=re.device)
    cov_im = torch.empty_like(cov_re)
    ctx.check(ctx.lib.gat_spatial_covariance(ctx._h, C.byref(desc), nb, bpe, _vp(cov_re), _vp(cov_im)), "gat_spatial_covariance")
    return torch.complex(cov_re, cov_im)


def _planes(z: torch.Tensor, dtype) -> tuple[torch.Tensor, torch.Tensor]:
    if z.is_complex():
        return z.real.to(dtype).contiguous(), z.imag.to(dtype).contiguous()
    return z.to(dtype).contiguous(), torch.zeros_like(z, dtype=dtype).contiguous()


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
        a_re, a_im = _planes(st.to(dev), torch.float64)
        K = int(st.shape[0])
    c_re = c_im = None
    if cov is not None:
        if cov.dim() != 2 or cov.shape[0] != cov.shape[1]:
            raise ValueError("cov must be [M, M] (pick one estimate of spatial_covariance)")
        c_re, c_im = _planes(cov, torch.float32)
    M = int(cov.shape[0] if cov is not None else a_re.shape[1])
    if a_re is not None and a_re.shape[1] != M:
        raise ValueError("steering and covariance disagree on the number of antennas")
    w_re = torch.empty((K, M), dtype=torch.float64, device=dev)
    w_im = torch.empty_like(w_re)
    ctx.check(ctx.lib.gat_array_weights(ctx._h, _vp(c_re), _vp(c_im), M, _vp(a_re), _vp(a_im), K, m, float(loading), _vp(w_re), _vp(w_im)),
              "gat_array_weights")
    return torch.complex(w_re, w_im)


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
    w_re, w_im = _planes(weights.to(acc_re.device), torch.float64)
    a_re, a_im = acc_re.contiguous(), acc_im.contiguous()
    y_re = torch.empty(shape[:-1], dtype=torch.float32, device=acc_re.device)
    y_im = torch.empty_like(y_re)
    ctx.check(ctx.lib.gat_beamform(ctx._h, _vp(a_re), _vp(a_im), B, K, L, M, _vp(w_re), _vp(w_im), _vp(y_re), _vp(y_im)), "gat_beamform")
    return y_re, y_im


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
    ostride = N if out_block_stride is None else int(out_block_stride)
    if ostride < N:
        raise ValueError("out_block_stride shorter than num_samples")
    w_re, w_im = _planes(w.to(ctx.device), torch.float64)
    ld = nb * ostride
    alloc = torch.zeros if zero else torch.empty
    if interleaved:
        out = alloc((J, ld, 2), dtype=torch.float32, device=ctx.device)
        odesc = _lib.SignalDesc(out.data_ptr(), None, _lib.GAT_LAYOUT_INTERLEAVED, J, N, ld, ostride, 0)
    else:
        out = (alloc((J, ld), dtype=torch.float32, device=ctx.device), alloc((J, ld), dtype=torch.float32, device=ctx.device))
        odesc = _lib.SignalDesc(out[0].data_ptr(), out[1].data_ptr(), _lib.GAT_LAYOUT_PLANAR, J, N, ld, ostride, 0)
    ctx.check(ctx.lib.gat_beamform_samples(ctx._h, C.byref(desc), nb, _vp(w_re), _vp(w_im), J, C.byref(odesc)), "gat_beamform_samples")
    return out, odesc


def beamform_samples(signal, weights: torch.Tensor, num_samples: int, num_blocks: int = 1, start: int = 0, block_stride: int | None = None,
                     out_block_stride: int | None = None, interleaved: bool = False, ctx: Context | None = None):
    """Beams of the raw samples, ``y[j, n] = sum_m conj(w[j, m]) x[m, n]`` for every sample of ``num_blocks`` blocks.
    ``signal`` as ``spatial_covariance`` takes it; ``weights`` complex (or real) ``[J, M]`` or ``[M]`` of any float dtype,
    moved to the float64 planes ``beamformer_weights`` returns.  Returns ``(re, im)`` float32 ``[J, num_blocks *
    out_block_stride]``, or with ``interleaved=True`` one tensor ``[J, num_blocks * out_block_stride, 2]``; block b starts
    ``b * out_block_stride`` samples in (default: ``num_samples``; what a larger stride leaves between blocks is zero: the
    allocation's, the kernel does not write there).  The result is a J-antenna signal for ``acquire``, ``spatial_covariance``
    and the correlators.  float32 sums in antenna order: ``|y - y64| <= (4 M + 4) 2^-24 sum_m |w_m| |x_m|``."""
    re, im = signal if isinstance(signal, (tuple, list)) else (signal, None)
    nb, N = int(num_blocks), int(num_samples)
    if nb < 1 or N < 1:
        raise ValueError("num_blocks and num_samples must be positive")
    stride = N if block_stride is None else int(block_stride)
    ntot = re.shape[-2] if im is None else re.shape[-1]
    if stride < 0 or start + (nb - 1) * stride + N > ntot:
        raise ValueError("signal shorter than start + (num_blocks - 1) * block_stride + num_samples")
    ctx = ctx if ctx is not None else get_context(re.device)
    desc = _signal_desc(re, im, N, start=int(start), block_stride=stride)
    return beamform_desc(ctx, desc, weights, nb, out_block_stride, interleaved)[0]
