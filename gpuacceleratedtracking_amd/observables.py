"""Observables (include/gat.h, "observables"): from what the loop tracked to what the position fix takes::

    acc_re, acc_im, history = loop.run_history(re, im, num_blocks)     # gat_tracking_run_history: every block's parameters
    mon = loop.monitor(acc_re, acc_im)                                 # bit synchronisation
    nav = loop.navigation(mon)                                         # frame synchronisation, TOW
    obs = loop.observables(history, mon, nav, epoch_stride=20)         # gat_observables: enqueued, not synchronised
    fix = position_fix(ephs, obs.tx_ms, obs.tx_frac, obs.rx_ms, obs.rx_frac)

``history`` is a uint8 device tensor ``[B + 1, K, 40]`` (``gat_channel_params`` records), the monitor's and the decoder's records
are passed where those calls wrote them: nothing is read back before the fix.  An ``Observables`` of the device call keeps device
tensors (``tx_ms``, ``tx_frac`` ``[E, K]``, ``rx_ms``, ``rx_frac`` ``[E]``, ``carrier_cycles``, ``carrier_frac``, ``doppler_hz``,
``code_rate_hz`` ``[E, K]``) and reads ``channels`` (status, frame_block, tow_frame, frame0_ms, edge_period, edge_fraction) back at the
first look.  ``observables_host`` is the host twin with the same bits over numpy arrays."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .monitor import TrackMonitor
from .navigation import NavResult, _format
from .results import PlannedResult, host_check, new_plan, plan_report, wanted
from .streams import addr, keep_alive, vp

BAD_RECORD, NO_BIT_SYNC, NO_FRAME_SYNC = _lib.GAT_OBS_BAD_RECORD, _lib.GAT_OBS_NO_BIT_SYNC, _lib.GAT_OBS_NO_FRAME_SYNC
FRAME_OUTSIDE, NO_TOW, EDGE_AMBIGUOUS = _lib.GAT_OBS_FRAME_OUTSIDE, _lib.GAT_OBS_NO_TOW, _lib.GAT_OBS_EDGE_AMBIGUOUS
OUTPUTS = ("tx_ms", "tx_frac", "rx_ms", "rx_frac", "carrier_cycles", "carrier_frac", "doppler_hz", "code_rate_hz", "channels")
_DTYPES = {"tx_ms": (torch.int32, np.int32), "rx_ms": (torch.int32, np.int32), "carrier_cycles": (torch.int64, np.int64)}


def obs_config(*, format, code_length: int, code_freq_nominal_hz: float, block_seconds: float, block_samples: int, sampling_freq_hz: float,
               symbol_blocks: int, max_frames: int, if_hz: float = 0.0, min_tow_steps: int = 0, epoch_first: int = 0, epoch_stride: int = 1,
               rx="from_tx", travel_ms: int = 68, edge_margin: float = 0.1) -> _lib.ObsConfig:
    """``gat_obs_config`` from Python values; ``rx``: "from_tx" or the reception ``(ms, frac)`` at block 0.  Nothing is checked: the
    library refuses."""
    cfg = _lib.ObsConfig()
    cfg.struct_size = C.sizeof(_lib.ObsConfig)
    cfg.format = format if isinstance(format, (int, np.integer)) else _format(format)
    cfg.code_length, cfg.symbol_blocks, cfg.block_samples = int(code_length), int(symbol_blocks), int(block_samples)
    cfg.code_freq_nominal_hz, cfg.block_seconds = float(code_freq_nominal_hz), float(block_seconds)
    cfg.sampling_freq_hz, cfg.if_hz = float(sampling_freq_hz), float(if_hz)
    cfg.max_frames, cfg.min_tow_steps = int(max_frames), int(min_tow_steps)
    cfg.epoch_first, cfg.epoch_stride, cfg.travel_ms, cfg.edge_margin = int(epoch_first), int(epoch_stride), int(travel_ms), float(edge_margin)
    if isinstance(rx, str):
        if rx != "from_tx":
            raise ValueError('rx must be "from_tx" or (ms, frac)')
        cfg.rx_mode = _lib.GAT_OBS_RX_FROM_TX
    else:
        cfg.rx_mode, cfg.rx0_ms, cfg.rx0_frac = _lib.GAT_OBS_RX_GIVEN, int(rx[0]), float(rx[1])
    return cfg


class Observables(PlannedResult):
    """The outputs of one call: the arrays that were asked for, as the call wrote them (device tensors of the device call, numpy
    arrays of the host twin) and, derived from ``channels`` on the host, ``status``, ``frame_block``, ``tow_frame``, ``frame0_ms``,
    ``edge_period``, ``edge_fraction`` ``[K]`` and ``measured``."""

    _VIEWS = {"channels": (_lib.OBS_CHANNEL_DTYPE, False)}

    def host(self, name: str) -> np.ndarray:
        """output ``name`` as a numpy array (synchronises a device call once)"""
        return self._h()[name]

    def __getattr__(self, name):
        if name in OUTPUTS:
            raw = self.__dict__["_raw"]
            if name not in raw:
                raise AttributeError(f"{name} was not asked for (outputs=)")
            return self._h()[name] if name == "channels" else raw[name]
        if name in _lib.OBS_CHANNEL_DTYPE.names:
            return self.channels[name].copy()
        raise AttributeError(name)

    @property
    def measured(self) -> np.ndarray:
        return (self.channels["status"] & ~EDGE_AMBIGUOUS) == 0


def _with_epochs(obs: Observables, cfg) -> Observables:
    """what the carrier smoothing reads of the call besides its arrays: ``if_hz`` and ``epoch_seconds`` = epoch_stride * block_seconds"""
    obs.if_hz, obs.epoch_seconds = float(cfg.if_hz), int(cfg.epoch_stride) * float(cfg.block_seconds)
    return obs


def _loop_config(loop, mon, config: dict) -> dict:
    """the loop's and the monitor's values under the caller's"""
    if loop is not None:
        lc = loop.config
        for name, value in (("block_seconds", lc.block_seconds), ("block_samples", loop.N), ("sampling_freq_hz", loop.fs),
                            ("code_length", lc.code_length), ("code_freq_nominal_hz", lc.code_freq_nominal_hz), ("if_hz", lc.if_hz),
                            ("format", loop.system)):
            config.setdefault(name, value)
    if isinstance(mon, TrackMonitor):
        config.setdefault("symbol_blocks", mon.symbol_blocks)
    return config


def _epochs(B: int, epoch_first: int, epoch_stride: int, num_epochs) -> int:
    if num_epochs is not None:
        return int(num_epochs)
    return (B - int(epoch_first)) // max(int(epoch_stride), 1) + 1 if int(epoch_first) <= B else 0


def _shape(name: str, E: int, K: int) -> tuple:
    return (E,) if name in ("rx_ms", "rx_frac") else (E, K)


def observables(history: torch.Tensor, mon, nav, *, loop=None, epoch_first: int = 0, epoch_stride: int = 1, num_epochs: int | None = None,
                rx="from_tx", outputs=None, ctx: Context | None = None, **config) -> Observables:
    """``gat_observables`` on the device.  ``history``: uint8 ``[B + 1, K, 40]`` (``TrackingLoop.run_history``); ``mon``: a
    ``TrackMonitor`` of the device call or its K channel records as a device tensor; ``nav``: a ``NavResult`` of the device call or
    ``(channels, frames)`` device tensors -- all passed as they are.  ``loop=`` fills block_seconds, block_samples,
    sampling_freq_hz, code_length, code_freq_nominal_hz, if_hz and the format; a monitor fills symbol_blocks; ``config`` takes the
    rest of ``obs_config``.  ``num_epochs`` None: every epoch up to record B.  Enqueues on the context's stream and returns at once."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    if not isinstance(history, torch.Tensor) or history.dtype != torch.uint8 or history.dim() != 3 or history.shape[2] != 40 or not history.is_contiguous():
        raise ValueError("history must be a contiguous uint8 device tensor [B + 1, K, 40]")
    B, K, dev = int(history.shape[0]) - 1, int(history.shape[1]), history.device
    mon_recs = mon._raw["channels"] if isinstance(mon, TrackMonitor) else mon
    nav_chan, nav_frames = (nav._raw["channels"], nav._raw["frames"]) if isinstance(nav, NavResult) else nav
    for name, t, size in (("mon", mon_recs, 32), ("nav channels", nav_chan, 32)):
        if not isinstance(t, torch.Tensor) or not t.is_contiguous() or t.device != dev or t.numel() * t.element_size() != K * size:
            raise ValueError(f"{name} must be the K records as a contiguous tensor on the device of history")
    if not isinstance(nav_frames, torch.Tensor) or not nav_frames.is_contiguous() or nav_frames.device != dev:
        raise ValueError("the frames must be a contiguous tensor on the device of history")
    frame_bytes = nav_frames.numel() * nav_frames.element_size()
    if frame_bytes % (K * 56) != 0:
        raise ValueError("the frames must be [K, max_frames] records of 56 bytes")
    config = _loop_config(loop, mon, dict(config))
    if isinstance(nav, NavResult):
        config.setdefault("format", nav.format)
    config.setdefault("max_frames", frame_bytes // (K * 56))
    if int(config["max_frames"]) * K * 56 > frame_bytes:
        raise ValueError("max_frames exceeds the rows of the frames")
    cfg = obs_config(epoch_first=epoch_first, epoch_stride=epoch_stride, rx=rx, **config)
    E = _epochs(B, epoch_first, epoch_stride, num_epochs)
    if ctx is None:
        ctx = loop.ctx if loop is not None else get_context(dev)
    raw = {}
    for name in want:
        if name == "channels":
            raw[name] = torch.empty((K, 32), dtype=torch.uint8, device=dev)
        else:
            raw[name] = torch.empty(_shape(name, max(E, 0), K), dtype=_DTYPES.get(name, (torch.float64,))[0], device=dev)
    rc = ctx.lib.gat_observables(ctx._h, vp(history), vp(mon_recs), vp(nav_chan), vp(nav_frames), B, K, E, C.byref(cfg),
                                 *[vp(raw.get(n)) for n in OUTPUTS])
    ctx.check(rc, "gat_observables")
    return keep_alive(_with_epochs(Observables(raw, ctx), cfg), history, mon_recs, nav_chan, nav_frames)


def observables_host(history, mon, nav, *, loop=None, epoch_first: int = 0, epoch_stride: int = 1, num_epochs: int | None = None,
                     rx="from_tx", outputs=None, **config) -> Observables:
    """``gat_observables_host``: the same rule and the same bits over numpy arrays; needs no device.  ``history``: a structured
    ``[B + 1, K]`` array of ``gat_channel_params`` (or uint8 ``[B + 1, K, 40]``); ``mon``: a ``TrackMonitor`` or its records; ``nav``: a
    ``NavResult`` or ``(channels, frames [K, max_frames])``."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    history = np.ascontiguousarray(history)
    if history.dtype != _lib.PARAMS_DTYPE:
        history = history.view(_lib.PARAMS_DTYPE).reshape(history.shape[0], -1)
    if history.ndim != 2:
        raise ValueError("history must be [B + 1, K]")
    B, K = history.shape[0] - 1, history.shape[1]
    mon_recs = np.ascontiguousarray(mon.channels if isinstance(mon, TrackMonitor) else mon)
    nav_chan, nav_frames = (nav.channels, nav.frames) if isinstance(nav, NavResult) else nav
    nav_chan, nav_frames = np.ascontiguousarray(nav_chan), np.ascontiguousarray(nav_frames)
    if mon_recs.nbytes != K * 32 or nav_chan.nbytes != K * 32 or nav_frames.nbytes % (K * 56) != 0:
        raise ValueError("mon and nav must hold K records each, the frames [K, max_frames] records")
    config = _loop_config(loop, mon, dict(config))
    if isinstance(nav, NavResult):
        config.setdefault("format", nav.format)
    config.setdefault("max_frames", nav_frames.nbytes // (K * 56))
    if int(config["max_frames"]) * K * 56 > nav_frames.nbytes:
        raise ValueError("max_frames exceeds the rows of the frames")
    cfg = obs_config(epoch_first=epoch_first, epoch_stride=epoch_stride, rx=rx, **config)
    E = _epochs(B, epoch_first, epoch_stride, num_epochs)
    raw = {}
    for name in want:
        if name == "channels":
            raw[name] = np.zeros(K, dtype=_lib.OBS_CHANNEL_DTYPE)
        else:
            raw[name] = np.zeros(_shape(name, max(E, 0), K), dtype=_DTYPES.get(name, (None, np.float64))[1])
    rc = _lib.load().gat_observables_host(addr(history), addr(mon_recs), addr(nav_chan), addr(nav_frames), B, K, E, C.byref(cfg),
                                          *[addr(raw.get(n)) for n in OUTPUTS])
    host_check(rc, "gat_observables_host")
    return _with_epochs(Observables(raw), cfg)


def observables_plan(num_blocks: int, num_channels: int, num_epochs: int | None = None, *, loop=None, epoch_first: int = 0, epoch_stride: int = 1,
                     rx="from_tx", **config) -> dict:
    """``gat_observables_plan``: the chunk length, the channel grouping, the workgroups of the kernels, their threads and LDS and the
    scratch bytes of such a call."""
    config = _loop_config(loop, None, dict(config))
    cfg = obs_config(epoch_first=epoch_first, epoch_stride=epoch_stride, rx=rx, **config)
    plan = new_plan(_lib.ObsPlan)
    E = _epochs(int(num_blocks), epoch_first, epoch_stride, num_epochs)
    rc = _lib.load().gat_observables_plan(int(num_blocks), int(num_channels), E, C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_observables_plan")
    return plan_report(plan)
