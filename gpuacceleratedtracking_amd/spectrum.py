"""The spectrum of the raw samples on device tensors (include/gat.h, "sample spectrum"): the summed periodogram per block and
antenna, the mean spectrum of a stream, a tone detector on it and the notch that needs no one to tell it where the tone is::

    psd, S = spectrum_stream((re, im), 1024, total)             # float64 [M, F]: mean power per bin
    tones = find_tones(psd)                                     # [(nu, dB over the floor), ...], strongest first
    y, desc, tones = auto_notch((re, im), total)                # ... and the stream behind one notch per tone
    results = acquire(system, desc, fs, prns)

The transform runs in libgat's HIP kernel; there is no CPU fallback (``sample_spectrum_host`` is the library's host twin, the
bit-exact reference of the device call, for tests and for machines without a GPU).  The bits of every block's sums are fixed by
the rule of gat.h.  ``spectrum_stream`` adds the blocks in float64 in block order: its last bits depend on how the stream was cut
into blocks, which the rule leaves to the caller.  ``find_tones`` works on the M * F numbers of the mean, on the host."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .filtering import filter_stream, notch_taps
from .streams import addr, input_desc, keep_alive, ref, vp

WINDOWS = ("hann", "hamming", "blackman", "rect")


def window_values(window, num_bins: int) -> np.ndarray:
    """float32 ``[F]``: a named window in its PERIODIC form (the DFT-even one, what a spectrum wants), computed in float64 and
    narrowed once, or a caller's F values narrowed."""
    F = int(num_bins)
    if isinstance(window, str):
        x = 2.0 * np.pi * np.arange(F, dtype=np.float64) / F
        if window == "hann":
            w = 0.5 - 0.5 * np.cos(x)
        elif window == "hamming":
            w = 0.54 - 0.46 * np.cos(x)
        elif window == "blackman":
            w = 0.42 - 0.5 * np.cos(x) + 0.08 * np.cos(2.0 * x)
        elif window == "rect":
            w = np.ones(F)
        else:
            raise ValueError(f"unknown window {window!r}")
        return w.astype(np.float32)
    w = np.asarray(window)
    if w.shape != (F,):
        raise ValueError(f"a window must hold num_bins = {F} values")
    return np.ascontiguousarray(w, dtype=np.float32)


def num_segments(num_samples: int, num_bins: int, hop: int) -> int:
    """``S = (N - F) / H + 1``: the segments of a block of ``num_samples``"""
    return (int(num_samples) - int(num_bins)) // int(hop) + 1


def _config(num_bins: int, hop: int, flags: int = 0) -> _lib.SpectrumConfig:
    return _lib.SpectrumConfig(C.sizeof(_lib.SpectrumConfig), int(num_bins), int(hop), int(flags))


def _hop(num_bins: int, hop) -> int:
    return int(num_bins) // 2 if hop is None else int(hop)


def sample_spectrum(signal, num_bins: int, num_samples: int, num_blocks: int = 1, hop: int | None = None, window="hann", start: int = 0,
                    block_stride: int | None = None, ctx: Context | None = None):
    """``power[b, m, f] = sum_s |FFT_F(w x[s H : s H + F])[f]|^2`` for every block of ``num_samples`` samples: float32 ``[B, M, F]``
    in FFT order (bin f is f / F cycles per sample below F / 2 and (f - F) / F above) -- the SUM over the ``S`` segments -- and S.
    ``signal`` as ``streams.input_desc`` takes it (any of the four layouts); ``hop`` defaults to F / 2; ``window``: a name of
    ``WINDOWS`` or F values."""
    F, H = int(num_bins), _hop(num_bins, hop)
    re, desc = input_desc(signal, num_samples, num_blocks, start, block_stride)
    if int(num_samples) < F or H < 1:
        raise ValueError("a block must hold one segment of num_bins samples, and hop must be positive")
    ctx = ctx if ctx is not None else get_context(re.device)
    w = torch.from_numpy(window_values(window, F)).to(re.device)
    out = torch.empty((int(num_blocks), int(desc.num_ants), F), dtype=torch.float32, device=re.device)
    cfg = _config(F, H)
    ctx.check(ctx.lib.gat_sample_spectrum(ctx._h, C.byref(desc), int(num_blocks), vp(w), C.byref(cfg), vp(out)), "gat_sample_spectrum")
    return keep_alive(out, w), num_segments(num_samples, F, H)


def sample_spectrum_host(desc: _lib.SignalDesc, num_blocks: int, window, num_bins: int, hop: int, out: np.ndarray | None,
                         config: _lib.SpectrumConfig | None = None) -> int:
    """``gat_sample_spectrum_host`` on a descriptor of HOST memory (``streams.host_desc`` builds one over numpy arrays) into
    ``out``, float32 ``[B, M, F]``.  Returns the status instead of raising: the refusals are part of what the twin is a reference
    of.  ``window``: float32 ``[F]`` or None (a null pointer); ``config`` overrides the one made of ``num_bins`` and ``hop``."""
    if window is not None and (window.dtype != np.float32 or not window.flags.c_contiguous):
        raise ValueError("window must be a contiguous float32 array")
    if out is not None and (out.dtype != np.float32 or not out.flags.c_contiguous):
        raise ValueError("out must be a contiguous float32 array")
    cfg = config if config is not None else _config(num_bins, hop)
    return int(_lib.load().gat_sample_spectrum_host(ref(desc), int(num_blocks), addr(window), C.byref(cfg), addr(out)))


def stream_partition(total_samples: int, num_bins: int, hop: int, num_ants: int, units_wanted: int = 2048):
    """How ``spectrum_stream`` cuts a stream of ``total_samples``: ``(S_total, S_block, B, S_rest)`` -- B blocks of ``S_block``
    segments every ``S_block * hop`` samples (``(S_block - 1) * hop + F`` samples each: neighbours overlap by F - hop), then one
    block of the ``S_rest`` segments left.  A (block, antenna) pair is the kernel's work unit and is never split, so B is what
    makes B * M reach ``units_wanted`` (eight workgroups a compute unit), within the segments there are and the 4096 a block holds."""
    F, H, M = int(num_bins), int(hop), int(num_ants)
    if int(total_samples) < F:
        raise ValueError("the stream is shorter than one segment")
    S_total = num_segments(total_samples, F, H)
    want_blocks = max(1, -(-int(units_wanted) // M))
    S_block = min(_lib.GAT_MAX_SPECTRUM_SEGMENTS, max(1, S_total // want_blocks))
    B = S_total // S_block
    return S_total, S_block, B, S_total - B * S_block


def spectrum_stream(signal, num_bins: int, total_samples: int, hop: int | None = None, window="hann", start: int = 0, ctx: Context | None = None,
                    units_wanted: int = 2048):
    """The mean power spectrum of one contiguous stream of ``total_samples``: float64 numpy ``[M, F]`` (FFT order) and the number
    of segments it is the mean of.  The stream is cut by descriptor into overlapping blocks (``stream_partition``) so that blocks
    x antennas cover the device; the blocks' float32 sums -- whose bits the rule of gat.h fixes -- are added in float64 in block
    order and divided by the segment count.  The last bits of the mean therefore depend on ``units_wanted``, nothing else does."""
    F, H = int(num_bins), _hop(num_bins, hop)
    re, desc = input_desc(signal, total_samples, 1, start, None)
    S_total, S_block, B, S_rest = stream_partition(total_samples, F, H, int(desc.num_ants), units_wanted)
    blocks, _ = sample_spectrum(signal, F, (S_block - 1) * H + F, B, H, window, start, S_block * H, ctx)
    total = blocks.cpu().numpy().astype(np.float64).sum(axis=0)  # (axis 0 of a C-ordered array: row after row, in block order)
    if S_rest:
        rest, _ = sample_spectrum(signal, F, (S_rest - 1) * H + F, 1, H, window, start + B * S_block * H, None, ctx)
        total = total + rest.cpu().numpy().astype(np.float64)[0]
    return total / S_total, S_total


def find_tones(psd, threshold_db: float = 10.0, max_tones: int = 4, guard_bins: int = 3, window="hann"):
    """CW tones in a mean spectrum ``[M, F]`` (or ``[F]``; numpy or torch, FFT order): ``[(nu, power_over_floor_db), ...]``,
    strongest first, ``nu`` in cycles per sample in [-1/2, 1/2).  The antennas are summed; the floor is the median over the bins;
    a tone is a local maximum (bins wrap around) more than ``threshold_db`` over the floor, and the ``guard_bins`` on either side
    of a tone taken hold no other.  With the "hann" window each maximum is refined by the two-bin estimator on magnitudes:
    ``alpha = sqrt(p[k +- 1] / p[k])`` toward the larger neighbour, ``delta = +-(2 alpha - 1) / (alpha + 1)``, ``nu = (k + delta) / F``;
    for any other window the bin centre is returned."""
    p = psd.detach().cpu().numpy() if isinstance(psd, torch.Tensor) else np.asarray(psd)
    p = p.astype(np.float64)
    p = p.sum(axis=0) if p.ndim == 2 else p
    if p.ndim != 1 or p.size < 4:
        raise ValueError("psd must be [M, F] or [F]")
    F = p.size
    floor = float(np.median(p))
    left, right = np.roll(p, 1), np.roll(p, -1)
    peaks = np.flatnonzero((p > left) & (p >= right) & (p > floor * 10.0 ** (float(threshold_db) / 10.0)))
    tones, taken = [], np.zeros(F, bool)
    for k in peaks[np.argsort(-p[peaks], kind="stable")]:
        if len(tones) >= int(max_tones):
            break
        near = (int(k) + np.arange(-int(guard_bins), int(guard_bins) + 1)) % F
        if taken[near].any():
            continue
        taken[near] = True
        delta = 0.0
        if isinstance(window, str) and window == "hann":
            up = right[k] >= left[k]
            alpha = np.sqrt((right[k] if up else left[k]) / p[k])
            delta = (2.0 * alpha - 1.0) / (alpha + 1.0) * (1.0 if up else -1.0)
        nu = (int(k) + delta) / F
        nu = (nu + 0.5) % 1.0 - 0.5
        tones.append((float(nu), float(10.0 * np.log10(p[k] / floor)) if floor > 0 else float("inf")))
    return tones


def auto_notch(signal, total_samples: int, num_bins: int = 1024, num_taps: int = 65, width: float = 0.01, threshold_db: float = 10.0,
               max_tones: int = 4, hop: int | None = None, guard_bins: int = 3, start: int = 0, num_blocks: int = 1, interleaved: bool = False,
               ctx: Context | None = None):
    """Find the CW tones of a stream and remove them, without being told where they are: ``spectrum_stream`` (Hann) ->
    ``find_tones`` -> the convolution of one ``notch_taps(num_taps, nu, width)`` per tone -> ``filter_stream``.  Returns
    ``(tensors, desc, tones)``: the filtered stream as ``filter_stream`` returns it (``total_samples - T + 1`` samples behind a
    filter of ``T = 1 + len(tones) * (num_taps - 1)`` taps, delayed by ``(T - 1) / 2`` samples), or -- no tone found -- the
    signal itself with the descriptor of its ``total_samples`` and ``tones == []``.  More tones than ``GAT_MAX_FIR_TAPS`` taps
    hold are refused."""
    psd, _ = spectrum_stream(signal, num_bins, total_samples, hop, "hann", start, ctx)
    tones = find_tones(psd, threshold_db, max_tones, guard_bins, "hann")
    if not tones:
        _, desc = input_desc(signal, total_samples, 1, start, None)
        return signal, desc, tones
    taps = np.ones(1, np.complex128)
    for nu, _ in tones:
        taps = np.convolve(taps, notch_taps(num_taps, nu, width))
    if taps.size > _lib.GAT_MAX_FIR_TAPS:
        raise ValueError(f"{len(tones)} notches of {num_taps} taps are a filter of {taps.size} taps: more than GAT_MAX_FIR_TAPS = {_lib.GAT_MAX_FIR_TAPS}")
    out, desc = filter_stream(signal, taps, total_samples, num_blocks=num_blocks, start=start, interleaved=interleaved, ctx=ctx)
    return out, desc, tones
