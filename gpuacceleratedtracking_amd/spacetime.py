"""Space-time adaptive processing on device tensors (include/gat.h, "space-time adaptive processing"): a tap delay line of
``T`` samples behind every antenna, all ``Q = M T`` coefficients solved at once, ``Q - 1`` degrees of freedom where the array
alone has ``M - 1``.  The snapshot of a block at sample ``n`` is ``z[t M + m] = x[m, n - t]`` (tap 0 the newest sample, the
antenna index fastest)::

    R = spacetime_covariance(signal, N, num_taps=5)[0]                       # [Q, Q], positive semi-definite by construction
    w = spacetime_weights(R, M, 5, ref_tap=2)                                # power inversion referenced to (tap 2, antenna 0)
    y, desc = spacetime_filter(signal, w, 5, N)                              # N - 4 samples: a 1-antenna signal
    results = acquire(system, desc, fs, prns)                                # code phases are those of sample d of x,
    d = spacetime_delay(5, 2)                                                # d = T - 1 - ref_tap = 2

The solver is ``beamformer_weights`` unchanged.  Everything runs in libgat's HIP kernels; there is no CPU fallback
(``spacetime_filter_host`` is the library's host twin, the bit-exact reference of the device call, for tests and for machines
without a GPU)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .array import beamformer_weights
from .context import Context, get_context
from .streams import addr, alloc_stream, input_desc, keep_alive, output_desc, overlap_save_blocks, planes, ref, stream_views, vp
from .streams import host_desc  # noqa: F401  (the name the host twin's docstring points to)


def spacetime_delay(num_taps: int, ref_tap: int) -> int:
    """``d = num_taps - 1 - ref_tap``: with weights referenced to tap ``ref_tap`` the filtered stream is the input ADVANCED by d
    samples -- output n' shows the wanted signal of input sample n' + d, so a code phase found on the output belongs to sample
    d of the input (and an event at input sample p appears at output sample p - d)."""
    T, r = int(num_taps), int(ref_tap)
    if not 0 <= r < T:
        raise ValueError("ref_tap must be in 0 .. num_taps - 1")
    return T - 1 - r


def spacetime_steering(a, num_taps: int, ref_tap: int) -> torch.Tensor:
    """The space-time steering vector ``a_st[t M + m] = a[m] [t == ref_tap]``, complex128 ``[K, M T]`` from ``a`` complex
    ``[K, M]`` or ``[M]``: with ``mode="mvdr"`` a distortionless response for direction ``a`` at ONE tap, so the wanted signal
    passes unfiltered, delayed by ``ref_tap`` samples."""
    T, r = int(num_taps), int(ref_tap)
    if not 0 <= r < T:
        raise ValueError("ref_tap must be in 0 .. num_taps - 1")
    a = torch.as_tensor(a)
    a = (a.reshape(1, -1) if a.dim() == 1 else a).to(torch.complex128)
    K, M = int(a.shape[0]), int(a.shape[1])
    st = torch.zeros((K, T, M), dtype=torch.complex128, device=a.device)
    st[:, r, :] = a
    return st.reshape(K, T * M)


def spacetime_covariance(signal, num_samples: int, num_blocks: int = 1, num_taps: int = 1, blocks_per_estimate: int | None = None,
                         start: int = 0, block_stride: int | None = None, ctx: Context | None = None) -> torch.Tensor:
    """``R_e[q, q'] = sum_{b in e} sum_{n = T-1}^{N-1} z_q[n] conj(z_q'[n])`` as complex64 ``[E, Q, Q]``, ``Q = M num_taps``: the
    covariance method -- every entry over the same ``N - T + 1`` snapshots, none reading outside its block.  ``signal`` as
    ``streams.input_desc`` takes it, the estimate grouping as in ``spatial_covariance``; ``num_taps = 1`` IS
    ``spatial_covariance`` (the same bits).  Exactly Hermitian, and the same bits on every call."""
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    nb, T = int(num_blocks), int(num_taps)
    bpe = nb if blocks_per_estimate is None else int(blocks_per_estimate)
    if bpe < 1 or T < 1:
        raise ValueError("blocks_per_estimate and num_taps must be positive")
    ctx = ctx if ctx is not None else get_context(re.device)
    E, Q = (nb + bpe - 1) // bpe, int(desc.num_ants) * T
    cov_re = torch.empty((E, Q, Q), dtype=torch.float32, device=re.device)
    cov_im = torch.empty_like(cov_re)
    ctx.check(ctx.lib.gat_spacetime_covariance(ctx._h, C.byref(desc), nb, bpe, T, vp(cov_re), vp(cov_im)), "gat_spacetime_covariance")
    return torch.complex(cov_re, cov_im)


def spacetime_weights(cov: torch.Tensor, num_ants: int, num_taps: int, steering=None, ref_tap: int | None = None, ref_ant: int = 0,
                      mode: str | None = None, loading: float = 0.0, ctx: Context | None = None) -> torch.Tensor:
    """Weights complex128 ``[K, Q]`` from one space-time covariance ``[Q, Q]``: a thin wrapper over ``beamformer_weights``.
    Without ``steering``: power inversion, referenced to (``ref_tap``, ``ref_ant``) -- (0, 0) is the solver's
    ``"power_inversion"``, any other reference its ``"mvdr"`` with the unit vector of that element.  With ``steering`` (complex
    ``[K, M]`` or ``[M]``): ``"mvdr"`` (or ``mode``) with ``spacetime_steering(steering, num_taps, ref_tap)``.  ``ref_tap``
    defaults to 0; the filtered stream is advanced by ``spacetime_delay(num_taps, ref_tap)`` samples."""
    M, T = int(num_ants), int(num_taps)
    r = 0 if ref_tap is None else int(ref_tap)
    if cov.dim() != 2 or int(cov.shape[0]) != M * T or int(cov.shape[1]) != M * T:
        raise ValueError("cov must be [num_ants * num_taps, num_ants * num_taps] (pick one estimate of spacetime_covariance)")
    if not 0 <= r < T or not 0 <= int(ref_ant) < M:
        raise ValueError("ref_tap / ref_ant outside the snapshot")
    if steering is None:
        if mode not in (None, "power_inversion"):
            raise ValueError("this mode needs a steering vector")
        if r == 0 and int(ref_ant) == 0:
            return beamformer_weights(cov, None, "power_inversion", loading, ctx)
        e = torch.zeros(M, dtype=torch.complex128, device=cov.device)
        e[int(ref_ant)] = 1.0
        return beamformer_weights(cov, spacetime_steering(e, T, r), "mvdr", loading, ctx)
    a = torch.as_tensor(steering).to(cov.device)
    if int(a.shape[-1]) != M:
        raise ValueError("steering must be [K, num_ants] or [num_ants]")
    return beamformer_weights(cov, spacetime_steering(a, T, r), "mvdr" if mode is None else mode, loading, ctx)


def _weight_planes(weights, Q: int, device):
    w = torch.as_tensor(weights)
    w = w.reshape(1, -1) if w.dim() == 1 else w
    if w.dim() != 2 or int(w.shape[1]) != Q:
        raise ValueError("weights must be [J, num_ants * num_taps] or [num_ants * num_taps]")
    return planes(w.to(device), torch.float64), int(w.shape[0])


def spacetime_filter(signal, weights, num_taps: int, num_samples: int, num_blocks: int = 1, start: int = 0, block_stride: int | None = None,
                     interleaved: bool = False, out=None, ctx: Context | None = None, out_block_stride: int | None = None):
    """``y[j, n'] = sum_q conj(w[j, q]) z_q[n' + T - 1]`` for every block of ``num_samples`` input samples, ``N - T + 1`` outputs a
    block.  ``signal`` as ``streams.input_desc`` takes it; ``weights`` complex ``[J, Q]`` or ``[Q]`` as ``spacetime_weights``
    returns them.  Returns ``(tensor(s), desc)`` as ``filter_samples`` does: a float32 ``(re, im)`` pair ``[J, Ntot]`` or, with
    ``interleaved=True``, one tensor ``[J, Ntot, 2]``, and its descriptor (it points into the tensor: keep both), a J-antenna
    signal for ``acquire``, ``spatial_covariance`` and the correlators.  float32 sums in q order: ``|y - y64| <= (4 Q + 4) 2^-24
    sum_q |w_q| |z_q|``; one tap gives ``beamform_samples``' bits."""
    T = int(num_taps)
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    nb, N, M = int(num_blocks), int(num_samples), int(desc.num_ants)
    if T < 1 or N < T:
        raise ValueError("num_taps must be positive and a block no shorter than the tap delay line")
    (w_re, w_im), J = _weight_planes(weights, M * T, re.device)
    No = N - T + 1
    ctx = ctx if ctx is not None else get_context(re.device)
    if out is None:
        out, odesc = alloc_stream(J, No, nb, re.device, planar=not interleaved)
    else:
        odesc = output_desc(out, No, out_block_stride)
    ctx.check(ctx.lib.gat_spacetime_filter(ctx._h, C.byref(desc), nb, vp(w_re), vp(w_im), T, J, C.byref(odesc)), "gat_spacetime_filter")
    return out, keep_alive(odesc, w_re, w_im)


def spacetime_filter_host(desc: _lib.SignalDesc, num_blocks: int, weights, num_taps: int, out_desc: _lib.SignalDesc,
                          num_beams: int | None = None) -> int:
    """``gat_spacetime_filter_host`` on descriptors of HOST memory (``host_desc`` builds one over numpy arrays).  Returns the
    status instead of raising: the refusals are part of what the twin is a reference of.  ``weights``: complex (or real) ``[J, Q]``
    or ``[Q]``, a pair of float64 planes (either may be None: a null pointer), or None."""
    if weights is None:
        w_re = w_im = None
    elif isinstance(weights, tuple):
        w_re, w_im = weights
    else:
        w = np.asarray(weights).astype(np.complex128)
        w = w.reshape(1, -1) if w.ndim == 1 else w
        w_re, w_im = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    plane = w_re if w_re is not None else w_im
    J = int(num_beams) if num_beams is not None else (int(plane.shape[0]) if plane is not None and plane.ndim == 2 else 1)
    return int(_lib.load().gat_spacetime_filter_host(ref(desc), int(num_blocks), addr(w_re), addr(w_im), int(num_taps), J, ref(out_desc)))


def stream_blocks(total_samples: int, num_taps: int, num_blocks: int = 1):
    """Overlap-save geometry of a contiguous stream of ``total_samples``: ``(N, in_stride, Qout, B, outputs)`` -- B blocks of N =
    Qout + T - 1 input samples every Qout samples give Qout outputs each, ``outputs = B Qout`` in all (the stream's own total - T
    + 1, rounded down to a multiple of B)."""
    if int(num_blocks) < 1 or int(num_taps) < 1 or int(total_samples) < int(num_taps):
        raise ValueError("num_blocks and num_taps must be positive and the stream no shorter than the tap delay line")
    return overlap_save_blocks(total_samples, num_taps, 1, num_blocks)


def spacetime_stream(signal, weights, num_taps: int, total_samples: int, num_blocks: int = 1, start: int = 0, interleaved: bool = False,
                     ctx: Context | None = None):
    """One contiguous stream of ``total_samples`` through the space-time filter as ``num_blocks`` overlapping blocks (overlap-save
    by descriptor: no carry state), written back to back: ONE seamless output of ``num_blocks * Qout`` samples whose bits do not
    depend on ``num_blocks``.  Returns ``(tensor(s), desc)``; the descriptor is one block of all the outputs."""
    N, stride, Qout, B, total_out = stream_blocks(total_samples, num_taps, num_blocks)
    re, desc = input_desc(signal, N, B, start, stride)
    w = torch.as_tensor(weights)
    J = 1 if w.dim() == 1 else int(w.shape[0])
    out = stream_views(alloc_stream(J, total_out, 1, re.device, planar=not interleaved)[0], total_out)
    _, odesc = spacetime_filter(signal, weights, num_taps, N, B, start, stride, interleaved, out, ctx, out_block_stride=Qout)
    odesc.num_samples, odesc.block_stride = total_out, total_out
    return out, odesc
