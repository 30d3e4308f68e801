"""Tracking monitor (include/gat.h, "tracking monitor"): what a receiver asks of its tracking channels, from the accumulator
history ``TrackingLoop.run(keep=True)`` leaves on the device::

    acc_re, acc_im = loop.run(re, im, 400)                       # [B, K, L, M] on the device
    mon = loop.monitor(acc_re, acc_im, first_block=0)            # gat_track_monitor: enqueued, not synchronised
    mon.cn0_nwpr, mon.cn0_m2m4                                   # dB-Hz per channel / per channel and window
    mon.phase_lock                                               # cos 2 phi per channel and window: near 1 in lock
    mon.symbol_offset, mon.synced                                # where the data-bit edges are, in stream blocks
    mon.bits                                                     # +-1 per symbol, up to the Costas loop's sign

The sums are libgat's HIP kernels (``monitor_accumulators``) or its host twin with the same bits (``monitor_accumulators_host``);
the decibels are made here, in numpy, from the raw sums.  A ``TrackMonitor`` of the device call keeps device tensors and reads
them back (after ``ctx.sync()``) at the first look at a value.

The bits carry the Costas loop's half-cycle ambiguity: the arctan discriminator locks to the carrier or to its negative, so all
bits of a channel may be inverted.  Frame synchronisation (a preamble) resolves it and is not part of this layer: it is
``navigation.decode_navigation`` / ``TrackingLoop.navigation``, which take a ``TrackMonitor`` as it is."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .results import PlannedResult, host_check, new_plan, plan_report
from .streams import addr, keep_alive, vp

NH10 = "0000110101"
NH20 = "00000100110101001110"


def overlay_for(system, component: str = "data") -> np.ndarray:
    """The blocks of one data symbol as +-1 int8, for 1 ms blocks: ``GPSL1`` twenty +1 (a 20 ms bit, no secondary code); ``GPSL5`` the
    Neuman-Hofman code NH10 of the data component I5, or NH20 of the pilot Q5 with ``component="pilot"``; a 0 bit is +1.
    ``system``: a ``GNSSSystem`` or its name."""
    name = system if isinstance(system, str) else system.name
    if component not in ("data", "pilot"):
        raise ValueError("component must be 'data' or 'pilot'")
    if name == "GPSL1":
        return np.ones(20, dtype=np.int8)
    if name == "GPSL5":
        return np.array([1 - 2 * int(ch) for ch in (NH10 if component == "data" else NH20)], dtype=np.int8)
    raise ValueError(f"no overlay known for {name!r}")


def monitor_config(num_taps: int, prompt_index: int, window_blocks: int, overlay, symbol_offset, first_block: int) -> _lib.MonitorConfig:
    """``gat_monitor_config`` from Python values (``symbol_offset=None``: search).  Nothing is checked: the library refuses."""
    ov = np.ones(20, dtype=np.int8) if overlay is None else np.asarray(overlay).astype(np.int8).reshape(-1)
    cfg = _lib.MonitorConfig()
    cfg.struct_size = C.sizeof(_lib.MonitorConfig)
    cfg.num_taps, cfg.prompt_index, cfg.window_blocks = int(num_taps), int(prompt_index), int(window_blocks)
    cfg.symbol_blocks = int(ov.size)
    cfg.symbol_offset = -1 if symbol_offset is None else int(symbol_offset)
    cfg.first_block = int(first_block)
    for i, v in enumerate(ov[:_lib.GAT_MAX_SYMBOL_BLOCKS]):
        cfg.overlay[i] = int(v)
    return cfg


class TrackMonitor(PlannedResult):
    """The monitor of one call.  Raw sums: ``windows`` (structured ``[K, NW]``: sum_p2, sum_p4, sum_d, sum_i, sum_q, blocks),
    ``energy`` ``[K, Pd]``, ``channels`` (structured ``[K]``), ``symbols`` complex ``[K, capacity]`` with ``wbp`` and ``num_symbols``
    ``[K]``, ``prompts`` complex ``[K, B]`` or None.  Derived: ``phase_lock``, ``cn0_m2m4`` ``[K, NW]``; ``symbol_offset`` (stream
    blocks, -1: none), ``start`` (the call's block of symbol 0), ``sync_ratio``, ``synced``, ``bits`` int8 ``[K, capacity]`` (0
    beyond ``num_symbols``), ``cn0_nwpr`` ``[K]``."""

    _VIEWS = {"windows": (_lib.MONITOR_WINDOW_DTYPE, True), "channels": (_lib.MONITOR_CHANNEL_DTYPE, False)}

    def __init__(self, raw: dict, block_seconds: float, symbol_blocks: int, min_sync_ratio: float, ctx: Context | None = None):
        super().__init__(raw, ctx)
        self.block_seconds, self.symbol_blocks, self.min_sync_ratio = float(block_seconds), int(symbol_blocks), float(min_sync_ratio)

    # ---- raw sums
    windows = property(lambda self: self._h()["windows"])
    energy = property(lambda self: self._h()["energy"])
    channels = property(lambda self: self._h()["channels"])
    wbp = property(lambda self: self._h()["sym_wbp"])

    @property
    def prompts(self):
        h = self._h()
        return h["prompt_re"] + 1j * h["prompt_im"] if "prompt_re" in h else None

    @property
    def symbols(self) -> np.ndarray:
        h = self._h()
        return h["sym_re"] + 1j * h["sym_im"]

    # ---- what the receiver asks
    @property
    def phase_lock(self) -> np.ndarray:
        w = self.windows
        with np.errstate(divide="ignore", invalid="ignore"):
            return w["sum_d"] / w["sum_p2"]

    @property
    def cn0_m2m4(self) -> np.ndarray:
        w = self.windows
        with np.errstate(divide="ignore", invalid="ignore"):
            n = w["blocks"].astype(np.float64)
            m2, m4 = w["sum_p2"] / n, w["sum_p4"] / n
            rad = 2.0 * m2 * m2 - m4
            pd = np.sqrt(np.where(rad > 0.0, rad, np.nan))
            ratio = pd / ((m2 - pd) * self.block_seconds)
            return 10.0 * np.log10(np.where(ratio > 0.0, ratio, np.nan))

    symbol_offset = property(lambda self: self.channels["symbol_offset"].copy())
    start = property(lambda self: self.channels["start"].copy())
    num_symbols = property(lambda self: self.channels["num_symbols"].copy())

    @property
    def sync_ratio(self) -> np.ndarray:
        ch = self.channels
        with np.errstate(divide="ignore", invalid="ignore"):
            return ch["e_max"] / ch["e_second"]

    @property
    def synced(self) -> np.ndarray:
        return (self.channels["start"] >= 0) & (self.sync_ratio >= self.min_sync_ratio)

    @property
    def bits(self) -> np.ndarray:
        h = self._h()
        valid = np.arange(h["sym_re"].shape[1])[None, :] < self.channels["num_symbols"][:, None]
        return np.where(valid, np.where(h["sym_re"] < 0.0, -1, 1), 0).astype(np.int8)

    @property
    def cn0_nwpr(self) -> np.ndarray:
        h, Pd = self._h(), self.symbol_blocks
        out = np.full(h["sym_re"].shape[0], np.nan)
        if Pd == 1:
            return out
        for k, n in enumerate(self.channels["num_symbols"]):
            if n < 1:
                continue
            with np.errstate(divide="ignore", invalid="ignore"):
                mu = float(np.mean((h["sym_re"][k, :n] ** 2 + h["sym_im"][k, :n] ** 2) / h["sym_wbp"][k, :n]))
            if 1.0 < mu < Pd:
                out[k] = 10.0 * np.log10((mu - 1.0) / ((Pd - mu) * self.block_seconds))
        return out


def _shapes(shape, stride0):
    if len(shape) != 4:
        raise ValueError("accumulators must be [B, K, L, M]")
    B, K, L, M = (int(v) for v in shape)
    return B, K, L, M, int(stride0) if B > 1 else K * L * M


def _weights_np(weights, K, M):
    if weights is None:
        return None, None
    w = np.asarray(weights).astype(np.complex128)
    if w.shape != (K, M):
        raise ValueError(f"weights must be [K, M] = [{K}, {M}]")
    return np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)


def monitor_accumulators(acc_re: torch.Tensor, acc_im: torch.Tensor, *, block_seconds: float, prompt_index: int, window_blocks: int = 20,
                         overlay=None, symbol_offset: int | None = None, first_block: int = 0, weights=None, keep_prompts: bool = False,
                         min_sync_ratio: float = 1.02, ctx: Context | None = None) -> TrackMonitor:
    """``gat_track_monitor`` on float32 device tensors ``[B, K, L, M]`` (each block contiguous; dimension 0 may be padded).
    ``overlay``: +-1 per block of a symbol (``overlay_for``; default twenty +1); ``symbol_offset``: None to search, else the
    known offset in stream blocks; ``first_block``: the stream's number of block 0; ``weights``: complex ``[K, M]`` as the
    beamformed loop's, or a pair of float64 device tensors.  Enqueues on the context's stream and returns at once."""
    if acc_re.dtype != torch.float32 or acc_im.dtype != torch.float32 or acc_re.shape != acc_im.shape or acc_re.stride() != acc_im.stride():
        raise ValueError("acc_re and acc_im must be float32 tensors of one shape and layout")
    B, K, L, M, stride = _shapes(acc_re.shape, acc_re.stride(0))
    if acc_re.stride()[1:] != (L * M, M, 1):
        raise ValueError("each block's accumulators must be contiguous [K, L, M]")
    ctx = ctx if ctx is not None else get_context(acc_re.device)
    cfg = monitor_config(L, prompt_index, window_blocks, overlay, symbol_offset, first_block)
    Pd, W = int(cfg.symbol_blocks), max(1, int(window_blocks))
    dev = acc_re.device
    if weights is None:
        w_re = w_im = None
    elif isinstance(weights, tuple):
        w_re, w_im = weights
    else:
        w = torch.as_tensor(weights).to(dev)
        if tuple(w.shape) != (K, M):
            raise ValueError(f"weights must be [K, M] = [{K}, {M}]")
        w_re = (w.real if w.is_complex() else w).to(torch.float64).contiguous()
        w_im = w.imag.to(torch.float64).contiguous() if w.is_complex() else torch.zeros_like(w_re)
    cap = B // max(Pd, 1)
    raw = {"windows": torch.empty((K, (B + W - 1) // W * 6), dtype=torch.float64, device=dev),
           "energy": torch.empty((K, Pd), dtype=torch.float64, device=dev),
           "channels": torch.empty((K, 4), dtype=torch.float64, device=dev)}
    for name in ("sym_re", "sym_im", "sym_wbp"):
        raw[name] = torch.empty((K, cap), dtype=torch.float64, device=dev)
    if keep_prompts:
        raw["prompt_re"] = torch.empty((K, B), dtype=torch.float64, device=dev)
        raw["prompt_im"] = torch.empty((K, B), dtype=torch.float64, device=dev)
    rc = ctx.lib.gat_track_monitor(ctx._h, vp(acc_re), vp(acc_im), stride, B, K, M, C.byref(cfg), vp(w_re), vp(w_im),
                                   vp(raw.get("prompt_re")), vp(raw.get("prompt_im")), vp(raw["windows"]), vp(raw["energy"]),
                                   vp(raw["channels"]), vp(raw["sym_re"]), vp(raw["sym_im"]), vp(raw["sym_wbp"]))
    ctx.check(rc, "gat_track_monitor")
    return keep_alive(TrackMonitor(raw, block_seconds, Pd, min_sync_ratio, ctx), acc_re, acc_im, w_re, w_im)


def monitor_accumulators_host(acc_re, acc_im, *, block_seconds: float, prompt_index: int, window_blocks: int = 20, overlay=None,
                              symbol_offset: int | None = None, first_block: int = 0, weights=None, keep_prompts: bool = False,
                              min_sync_ratio: float = 1.02) -> TrackMonitor:
    """``gat_track_monitor_host``: the same rule and the same bits over float32 numpy arrays ``[B, K, L, M]``; needs no device."""
    acc_re, acc_im = np.ascontiguousarray(acc_re, dtype=np.float32), np.ascontiguousarray(acc_im, dtype=np.float32)
    if acc_re.shape != acc_im.shape:
        raise ValueError("acc_re and acc_im must have one shape")
    B, K, L, M, stride = _shapes(acc_re.shape, int(np.prod(acc_re.shape[1:])))
    cfg = monitor_config(L, prompt_index, window_blocks, overlay, symbol_offset, first_block)
    Pd, W = int(cfg.symbol_blocks), max(1, int(window_blocks))
    w_re, w_im = _weights_np(weights, K, M)
    cap = B // max(Pd, 1)
    raw = {"windows": np.zeros((K, (B + W - 1) // W), dtype=_lib.MONITOR_WINDOW_DTYPE), "energy": np.zeros((K, Pd)),
           "channels": np.zeros(K, dtype=_lib.MONITOR_CHANNEL_DTYPE)}
    for name in ("sym_re", "sym_im", "sym_wbp"):
        raw[name] = np.zeros((K, cap))
    if keep_prompts:
        raw["prompt_re"], raw["prompt_im"] = np.zeros((K, B)), np.zeros((K, B))
    rc = _lib.load().gat_track_monitor_host(addr(acc_re), addr(acc_im), stride, B, K, M, C.byref(cfg), addr(w_re), addr(w_im),
                                            addr(raw.get("prompt_re")), addr(raw.get("prompt_im")), addr(raw["windows"]), addr(raw["energy"]),
                                            addr(raw["channels"]), addr(raw["sym_re"]), addr(raw["sym_im"]), addr(raw["sym_wbp"]))
    host_check(rc, "gat_track_monitor_host")
    return TrackMonitor(raw, block_seconds, Pd, min_sync_ratio)


def monitor_plan(num_blocks: int, num_channels: int, num_ants: int, num_taps: int, prompt_index: int, window_blocks: int = 20, overlay=None,
                 symbol_offset: int | None = None, first_block: int = 0, acc_block_stride: int | None = None, own_prompts: bool = True,
                 want_symbols: bool = True) -> dict:
    """``gat_track_monitor_plan``: the counts, the scratch bytes and the workgroups of each kernel of such a call."""
    cfg = monitor_config(num_taps, prompt_index, window_blocks, overlay, symbol_offset, first_block)
    stride = int(num_channels) * int(num_taps) * int(num_ants) if acc_block_stride is None else int(acc_block_stride)
    plan = new_plan(_lib.MonitorPlan)
    rc = _lib.load().gat_track_monitor_plan(stride, int(num_blocks), int(num_channels), int(num_ants), C.byref(cfg), int(own_prompts),
                                            int(want_symbols), C.byref(plan))
    host_check(rc, "gat_track_monitor_plan")
    return plan_report(plan)
