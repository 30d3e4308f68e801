"""Subspace processing (include/gat.h, "subspace"): the covariance of the accumulator history, a batched Hermitian eigensolver
and, built from the two, the steering vector of every tracking channel as the receiver's own hardware sees it::

    acc_re, acc_im = loop.run(re, im, 400)                       # [B, K, L, M] on the device, a loop on antenna 0 or on any beam
    a, lam = loop.steering(acc_re, acc_im)                       # [E, K, M] complex128 and the eigenvalues [E, K, M], on the device
    w = beamformer_weights(None, a[0], "conventional")           # what TrackingLoop(weights=w) takes

An uncalibrated array knows neither its cable phases nor its geometry.  The prompt accumulators of a channel are ``A a + noise``
per block; their covariance over the blocks is ``|A|^2 a a^H + noise`` -- the data bits and the loop's common phase error cancel
in the outer product -- and its principal eigenvector is ``a``: the eigenbeamformer.  The eigenvalues say how many sources a
covariance holds (``source_count``, Wax-Kailath).

The sums and the Jacobi iteration are libgat's HIP kernels or its host twins with the same bits; there is no CPU fallback.  The
device calls enqueue on the context's stream and do not synchronise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .results import host_check, new_plan, plan_report
from .streams import addr, keep_alive, planes, vp


def _complex(re: np.ndarray, im: np.ndarray) -> np.ndarray:
    """the planes as one complex128 array, every bit kept (``re + 1j * im`` would turn a -0 real part into +0)"""
    z = np.empty(re.shape, dtype=np.complex128)
    z.real, z.imag = re, im
    return z


def _acc_shape(shape, stride0):
    if len(shape) != 4:
        raise ValueError("accumulators must be [B, K, L, M]")
    B, K, L, M = (int(v) for v in shape)
    return B, K, L, M, int(stride0) if B > 1 else K * L * M


def _estimates(B: int, blocks_per_estimate) -> tuple[int, int]:
    """(the argument of the C call, E)"""
    if blocks_per_estimate is None:
        return 0, 1
    bpe = int(blocks_per_estimate)
    if bpe < 1:
        raise ValueError("blocks_per_estimate must be positive")
    per = max(1, min(bpe, B))  # more than B: one estimate of all blocks
    return bpe, (B + per - 1) // per


def accumulator_covariance(acc_re: torch.Tensor, acc_im: torch.Tensor, *, tap_index: int, blocks_per_estimate: int | None = None,
                           ctx: Context | None = None) -> torch.Tensor:
    """``gat_accumulator_covariance``: ``R[e, k] = sum_{b in e} x_b x_b^H`` with ``x_b = acc[b, k, tap_index, :]``, complex128
    ``[E, K, M, M]`` on the device, from float32 device tensors ``[B, K, L, M]`` (each block contiguous; dimension 0 may be
    padded).  ``E = ceil(B / blocks_per_estimate)`` (None: one estimate of all blocks).  Exactly Hermitian; the same bits on every
    call and as ``accumulator_covariance_host``."""
    if acc_re.dtype != torch.float32 or acc_im.dtype != torch.float32 or acc_re.shape != acc_im.shape or acc_re.stride() != acc_im.stride():
        raise ValueError("acc_re and acc_im must be float32 tensors of one shape and layout")
    B, K, L, M, stride = _acc_shape(acc_re.shape, acc_re.stride(0))
    if acc_re.stride()[1:] != (L * M, M, 1):
        raise ValueError("each block's accumulators must be contiguous [K, L, M]")
    bpe, E = _estimates(B, blocks_per_estimate)
    ctx = ctx if ctx is not None else get_context(acc_re.device)
    cov_re = torch.empty((E, K, M, M), dtype=torch.float64, device=acc_re.device)
    cov_im = torch.empty_like(cov_re)
    ctx.check(ctx.lib.gat_accumulator_covariance(ctx._h, vp(acc_re), vp(acc_im), stride, B, K, L, M, int(tap_index), bpe, vp(cov_re), vp(cov_im)),
              "gat_accumulator_covariance")
    return keep_alive(torch.complex(cov_re, cov_im), acc_re, acc_im, cov_re, cov_im)


def accumulator_covariance_host(acc_re, acc_im, *, tap_index: int, blocks_per_estimate: int | None = None) -> np.ndarray:
    """``gat_accumulator_covariance_host``: the same rule and the same bits over float32 numpy arrays ``[B, K, L, M]``; needs no device."""
    acc_re, acc_im = np.ascontiguousarray(acc_re, dtype=np.float32), np.ascontiguousarray(acc_im, dtype=np.float32)
    if acc_re.shape != acc_im.shape:
        raise ValueError("acc_re and acc_im must have one shape")
    B, K, L, M, stride = _acc_shape(acc_re.shape, int(np.prod(acc_re.shape[1:])))
    bpe, E = _estimates(B, blocks_per_estimate)
    cov_re, cov_im = np.zeros((E, K, M, M)), np.zeros((E, K, M, M))
    rc = _lib.load().gat_accumulator_covariance_host(addr(acc_re), addr(acc_im), stride, B, K, L, M, int(tap_index), bpe, addr(cov_re), addr(cov_im))
    host_check(rc, "gat_accumulator_covariance_host")
    return _complex(cov_re, cov_im)


def _eig_shape(shape, num_vectors):
    if len(shape) < 2 or shape[-1] != shape[-2]:
        raise ValueError("cov must be [..., Q, Q]")
    Q = int(shape[-1])
    lead = tuple(int(v) for v in shape[:-2])
    n = int(np.prod(lead)) if lead else 1
    R = Q if num_vectors is None else int(num_vectors)
    return lead, n, Q, R


def hermitian_eig(cov: torch.Tensor, num_vectors: int | None = None, ctx: Context | None = None):
    """``gat_hermitian_eig`` of complex64 or complex128 ``[..., Q, Q]`` on the device (only the lower triangles and the diagonals'
    real parts are read): ``(eigenvalues [..., Q] descending, vectors [..., R, Q] complex128 with row r the eigenvector of
    eigenvalue r, status [...] int32)``, all on the device; ``R = num_vectors`` (None: all Q).  Each eigenvector's largest
    component is real and positive.  status: the sweeps used, -1 not converged, -2 a non-finite input (NaN outputs)."""
    if not cov.is_complex():
        raise ValueError("cov must be complex64 or complex128")
    lead, n, Q, R = _eig_shape(cov.shape, num_vectors)
    f32 = cov.dtype == torch.complex64
    a_re, a_im = planes(cov, torch.float32 if f32 else torch.float64)
    dev = cov.device
    ctx = ctx if ctx is not None else get_context(dev)
    lam = torch.empty(lead + (Q,), dtype=torch.float64, device=dev)
    v_re = torch.empty(lead + (R, Q), dtype=torch.float64, device=dev)
    v_im = torch.empty_like(v_re)
    status = torch.empty(lead, dtype=torch.int32, device=dev)
    ctx.check(ctx.lib.gat_hermitian_eig(ctx._h, vp(a_re), vp(a_im), n, Q, R, _lib.GAT_EIG_INPUT_F32 if f32 else 0, vp(lam), vp(v_re), vp(v_im),
                                        vp(status)), "gat_hermitian_eig")
    return keep_alive((lam, torch.complex(v_re, v_im), status), a_re, a_im, v_re, v_im)


def hermitian_eig_host(cov, num_vectors: int | None = None):
    """``gat_hermitian_eig_host``: the same rule and the same bits over a complex64 or complex128 numpy array; needs no device."""
    cov = np.asarray(cov)
    if cov.dtype not in (np.complex64, np.complex128):
        raise ValueError("cov must be complex64 or complex128")
    lead, n, Q, R = _eig_shape(cov.shape, num_vectors)
    f32 = cov.dtype == np.complex64
    part = np.float32 if f32 else np.float64
    a_re, a_im = np.ascontiguousarray(cov.real, dtype=part), np.ascontiguousarray(cov.imag, dtype=part)
    lam, v_re, v_im = np.zeros(lead + (Q,)), np.zeros(lead + (R, Q)), np.zeros(lead + (R, Q))
    status = np.zeros(lead, dtype=np.int32)
    rc = _lib.load().gat_hermitian_eig_host(addr(a_re), addr(a_im), n, Q, R, _lib.GAT_EIG_INPUT_F32 if f32 else 0, addr(lam), addr(v_re), addr(v_im),
                                            addr(status))
    host_check(rc, "gat_hermitian_eig_host")
    return lam, _complex(v_re, v_im), status


def steering_from_accumulators(acc_re: torch.Tensor, acc_im: torch.Tensor, *, tap_index: int, ref_ant: int = 0,
                               blocks_per_estimate: int | None = None, ctx: Context | None = None):
    """``(steering [E, K, M] complex128, eigenvalues [E, K, M])`` on the device: the principal eigenvector of every channel's
    accumulator covariance, re-phased so that component ``ref_ant`` is real and not negative (a zero component is left as it is).
    ``steering[e]`` goes straight into ``beamformer_weights``."""
    M = int(acc_re.shape[-1])
    if not 0 <= int(ref_ant) < M:
        raise ValueError("ref_ant outside the antennas")
    cov = accumulator_covariance(acc_re, acc_im, tap_index=tap_index, blocks_per_estimate=blocks_per_estimate, ctx=ctx)
    lam, vec, _ = hermitian_eig(cov, 1, ctx=ctx)
    a = vec[..., 0, :]
    r = a[..., int(ref_ant)]
    mod = r.abs()
    one = torch.ones_like(r)
    factor = torch.where(mod > 0, r.conj() / torch.where(mod > 0, mod, torch.ones_like(mod)), one)
    return a * factor.unsqueeze(-1), lam


def subspace_plan(num_blocks: int = 0, num_channels: int = 1, num_taps: int = 1, num_ants: int = 1, tap_index: int = 0,
                  blocks_per_estimate: int | None = None, acc_block_stride: int | None = None, eig_matrices: int = 0, eig_order: int = 1,
                  eig_vectors: int | None = None) -> dict:
    """``gat_subspace_plan``: the estimates, the chunks, the work split, the scratch bytes and the workgroups of
    ``accumulator_covariance`` (``num_blocks`` > 0) and of ``hermitian_eig`` (``eig_matrices`` > 0) for such calls."""
    stride = int(num_channels) * int(num_taps) * int(num_ants) if acc_block_stride is None else int(acc_block_stride)
    plan = new_plan(_lib.SubspacePlan)
    rc = _lib.load().gat_subspace_plan(stride, int(num_blocks), int(num_channels), int(num_taps), int(num_ants), int(tap_index),
                                       0 if blocks_per_estimate is None else int(blocks_per_estimate), int(eig_matrices), int(eig_order),
                                       int(eig_order) if eig_vectors is None else int(eig_vectors), C.byref(plan))
    host_check(rc, "gat_subspace_plan")
    return plan_report(plan)


def source_count(eigenvalues, num_snapshots: int, method: str = "mdl"):
    """The number of sources in a covariance of ``num_snapshots`` snapshots from its eigenvalues ``[..., Q]`` (any order), by the
    information criteria of Wax and Kailath (1985).  With l_1 >= .. >= l_Q and, for k sources, the arithmetic mean a_k and the
    geometric mean g_k of the Q - k smallest: ``L(k) = N (Q - k) ln(a_k / g_k)``, ``AIC(k) = 2 L(k) + 2 k (2 Q - k)``,
    ``MDL(k) = L(k) + k (2 Q - k) ln(N) / 2``; the count is the k in 0 .. Q-1 with the smallest criterion (the lowest of equals).
    Runs on the host in numpy; eigenvalues that are not positive count as the smallest positive double.  An int, or an int array
    ``[...]``."""
    if method not in ("mdl", "aic"):
        raise ValueError("method must be 'mdl' or 'aic'")
    N = int(num_snapshots)
    if N < 1:
        raise ValueError("num_snapshots must be positive")
    lam = eigenvalues.detach().cpu().numpy() if isinstance(eigenvalues, torch.Tensor) else np.asarray(eigenvalues)
    lam = np.sort(np.maximum(lam.astype(np.float64), np.finfo(np.float64).tiny), axis=-1)[..., ::-1]
    Q = lam.shape[-1]
    crit = np.empty(lam.shape[:-1] + (Q,))
    for k in range(Q):
        tail = lam[..., k:]
        like = N * (Q - k) * (np.log(tail.mean(axis=-1)) - np.log(tail).mean(axis=-1))
        free = k * (2 * Q - k)
        crit[..., k] = 2.0 * like + 2.0 * free if method == "aic" else like + 0.5 * free * np.log(N)
    out = np.argmin(crit, axis=-1)
    return int(out) if out.ndim == 0 else out
