"""Carrier smoothing (include/gat.h, "carrier smoothing"): the observables' code-phase transmit times smoothed by their carrier
phase over the last ``window`` epochs of an arc, arcs cut at gaps and cycle slips::

    obs = loop.observables(history, mon, nav, epoch_stride=20)         # gat_observables
    sm = smooth_observables(obs, window=100)                           # gat_smooth_observables: enqueued, not synchronised
    fix = position_fix(ephs, obs.tx_ms, sm.tx_frac_dev, obs.rx_ms, obs.rx_frac)
    sm.count, sm.cmc_m, sm.status, sm.channels                         # read back at the first look

observables -> smooth -> fix -> corrections -> fix (or RAIM) -> velocity runs with nothing read back.  The work is libgat's HIP
kernels (``smooth_observables``) or their host twin with the same bits (``smooth_observables_host``).  White code noise of sigma
leaves sigma / sqrt(n) after n epochs of an arc, n <= window; the window bounds what the ionosphere's code-carrier divergence
(twice its rate of change) adds."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .observables import Observables
from .results import PlannedResult, host_check, new_plan, plan_report, wanted
from .streams import addr, keep_alive, vp

RATE_TEST = _lib.GAT_SMOOTH_RATE_TEST
MEASURED, GAP, CMC, RATE = _lib.GAT_SMOOTH_MEASURED, _lib.GAT_SMOOTH_GAP, _lib.GAT_SMOOTH_CMC, _lib.GAT_SMOOTH_RATE
OUTPUTS = ("count", "cmc_s", "status", "channels")
_DTYPES = {"count": (torch.int32, np.int32), "cmc_s": (torch.float64, np.float64), "status": (torch.uint8, np.uint8)}
_INPUTS = ("tx_ms", "tx_frac", "rx_ms", "rx_frac", "carrier_cycles", "carrier_frac")
_IN_DTYPES = {"tx_ms": "int32", "tx_frac": "float64", "rx_ms": "int32", "rx_frac": "float64", "carrier_cycles": "int64",
              "carrier_frac": "float64", "doppler_hz": "float64", "valid": "uint8"}
C_LIGHT = 299792458.0


def smooth_config(*, window: int, if_hz: float, epoch_seconds: float, cmc_gate_s: float, rate_gate_cycles: float | None = None,
                  carrier_hz: float = 1575.42e6, flags: int | None = None) -> _lib.SmoothConfig:
    """``gat_smooth_config`` from Python values; ``rate_gate_cycles`` None: no rate test.  Nothing is checked: the library refuses."""
    cfg = _lib.SmoothConfig()
    cfg.struct_size = C.sizeof(_lib.SmoothConfig)
    cfg.flags = (RATE_TEST if rate_gate_cycles is not None else 0) if flags is None else int(flags)
    cfg.window, cfg.reserved = int(window), 0
    cfg.carrier_hz, cfg.if_hz, cfg.epoch_seconds = float(carrier_hz), float(if_hz), float(epoch_seconds)
    cfg.cmc_gate_s = float(cmc_gate_s)
    cfg.rate_gate_cycles = 0.0 if rate_gate_cycles is None else float(rate_gate_cycles)
    return cfg


class SmoothedObservables(PlannedResult):
    """The outputs of one call.  ``tx_frac_dev`` is ``tx_frac_out`` float64 ``[E, K]`` as the call left it (a device tensor of the
    device call), to pass on without a look; ``tx_frac_out`` / ``tx_frac`` the same on the host.  Where asked for: ``count`` int32
    ``[E, K]`` (the n used), ``cmc_s`` float64 ``[E, K]`` (code minus carrier since the arc began; ``cmc_m`` in metres), ``status``
    uint8 ``[E, K]`` (MEASURED, GAP, CMC, RATE) and ``channels`` ``[K]`` (measured, arcs, cmc_resets, rate_resets, each also an
    attribute)."""

    _VIEWS = {"channels": (_lib.SMOOTH_CHANNEL_DTYPE, False)}

    def __getattr__(self, name):
        if name in OUTPUTS:
            if name not in self.__dict__["_raw"]:
                raise AttributeError(f"{name} was not asked for (outputs=)")
            return self._h()[name]
        if name in _lib.SMOOTH_CHANNEL_DTYPE.names:
            return self.channels[name].copy()
        raise AttributeError(name)

    tx_frac_dev = property(lambda self: self._raw["tx_frac_out"])
    tx_frac_out = property(lambda self: self._h()["tx_frac_out"])
    tx_frac = tx_frac_out
    cmc_m = property(lambda self: self.cmc_s * C_LIGHT, doc="float64 [E, K]: m")
    arc_start = property(lambda self: (self.status & (GAP | CMC | RATE)) != 0)


def _inputs(obs, tx_frac, if_hz, epoch_seconds, rate: bool):
    """the arrays of a call by name (as ``obs`` holds them; its Doppler with the rate test, where it has one: the library refuses
    the test without) and the two values derived from it"""
    if not isinstance(obs, Observables):
        raise TypeError("obs must be an Observables (observables / observables_host)")
    raw = obs._raw
    missing = [n for n in _INPUTS if n not in raw and not (n == "tx_frac" and tx_frac is not None)]
    if missing:
        raise ValueError(f"the observables were made without {missing} (outputs=)")
    arrays = {n: raw[n] for n in _INPUTS + (("doppler_hz",) if rate else ()) if n in raw}
    if tx_frac is not None:
        arrays["tx_frac"] = tx_frac
    if_hz = getattr(obs, "if_hz", None) if if_hz is None else if_hz
    epoch_seconds = getattr(obs, "epoch_seconds", None) if epoch_seconds is None else epoch_seconds
    if if_hz is None or epoch_seconds is None:
        raise ValueError("these observables do not say their if_hz and epoch_seconds: pass both")
    return arrays, float(if_hz), float(epoch_seconds)


def smooth_observables(obs: Observables, *, window: int, cmc_gate_m: float = 15.0, rate_gate_cycles: float | None = None, valid=None,
                       carrier_hz: float = 1575.42e6, tx_frac=None, if_hz: float | None = None, epoch_seconds: float | None = None,
                       outputs=None, ctx: Context | None = None, flags: int | None = None) -> SmoothedObservables:
    """``gat_smooth_observables`` on the device.  ``obs``: the ``Observables`` of the device call, its tensors passed as they are;
    ``if_hz`` and ``epoch_seconds`` (epoch_stride * block_seconds) are its own where not given.  ``window``: W epochs; ``cmc_gate_m``:
    the gate on the growth of code minus carrier between two epochs, in metres (at most c 2^-18 s = 1143 m); ``rate_gate_cycles``:
    the gate of the rate test against ``doppler_hz`` (None: no rate test); ``valid``: a uint8 device tensor ``[E, K]``, 0 = not
    measured; ``tx_frac``: a float64 device tensor ``[E, K]`` in place of the observables' (the atmosphere's ``tx_frac_dev``).
    ``outputs``: which of "count", "cmc_s", "status", "channels" to write (None: all).  Enqueues on the context's stream and returns
    at once."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    need_doppler = rate_gate_cycles is not None or bool((flags or 0) & RATE_TEST)
    a, if_hz, epoch_seconds = _inputs(obs, tx_frac, if_hz, epoch_seconds, need_doppler)
    if valid is not None:
        a["valid"] = valid
    tx_ms = a["tx_ms"]
    if not isinstance(tx_ms, torch.Tensor) or tx_ms.dim() != 2:
        raise ValueError("obs must be the Observables of the device call (observables)")
    E, K, dev = int(tx_ms.shape[0]), int(tx_ms.shape[1]), tx_ms.device
    for name, t in a.items():
        shape = (E,) if name in ("rx_ms", "rx_frac") else (E, K)
        if not isinstance(t, torch.Tensor) or t.dtype != getattr(torch, _IN_DTYPES[name]) or tuple(t.shape) != shape or not t.is_contiguous() \
                or t.device != dev:
            raise ValueError(f"{name} must be a contiguous {_IN_DTYPES[name]} tensor {list(shape)} on the device of tx_ms")
    if ctx is None:
        ctx = obs._ctx if obs._ctx is not None else get_context(dev)
    cfg = smooth_config(window=window, if_hz=if_hz, epoch_seconds=epoch_seconds, cmc_gate_s=float(cmc_gate_m) / C_LIGHT,
                        rate_gate_cycles=rate_gate_cycles, carrier_hz=carrier_hz, flags=flags)
    raw = {"tx_frac_out": torch.empty((E, K), dtype=torch.float64, device=dev)}
    for name in want:
        raw[name] = torch.empty((K, 16), dtype=torch.uint8, device=dev) if name == "channels" else torch.empty((E, K), dtype=_DTYPES[name][0], device=dev)
    rc = ctx.lib.gat_smooth_observables(ctx._h, *[vp(a.get(n)) for n in _INPUTS + ("doppler_hz", "valid")], E, K, C.byref(cfg),
                                        vp(raw["tx_frac_out"]), *[vp(raw.get(n)) for n in OUTPUTS])
    ctx.check(rc, "gat_smooth_observables")
    return keep_alive(SmoothedObservables(raw, ctx), *a.values())


def smooth_observables_host(obs: Observables, *, window: int, cmc_gate_m: float = 15.0, rate_gate_cycles: float | None = None, valid=None,
                            carrier_hz: float = 1575.42e6, tx_frac=None, if_hz: float | None = None, epoch_seconds: float | None = None,
                            outputs=None, flags: int | None = None) -> SmoothedObservables:
    """``gat_smooth_observables_host``: the same rule and the same bits over numpy arrays; needs no device.  ``obs``: an
    ``Observables`` of either call (a device call's is read back); ``valid``, ``tx_frac``: arrays ``[E, K]``."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    need_doppler = rate_gate_cycles is not None or bool((flags or 0) & RATE_TEST)
    a, if_hz, epoch_seconds = _inputs(obs, tx_frac, if_hz, epoch_seconds, need_doppler)
    host = obs._h()
    a = {n: (host[n] if v is obs._raw.get(n) else v) for n, v in a.items()}
    if valid is not None:
        a["valid"] = valid
    a = {n: np.ascontiguousarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=_IN_DTYPES[n]) for n, v in a.items()}
    if a["tx_ms"].ndim != 2:
        raise ValueError("tx_ms must be [E, K]")
    E, K = a["tx_ms"].shape
    for name, v in a.items():
        if v.shape != ((E,) if name in ("rx_ms", "rx_frac") else (E, K)):
            raise ValueError(f"{name} has the wrong shape")
    cfg = smooth_config(window=window, if_hz=if_hz, epoch_seconds=epoch_seconds, cmc_gate_s=float(cmc_gate_m) / C_LIGHT,
                        rate_gate_cycles=rate_gate_cycles, carrier_hz=carrier_hz, flags=flags)
    raw = {"tx_frac_out": np.zeros((E, K), dtype=np.float64)}
    for name in want:
        raw[name] = np.zeros(K, dtype=_lib.SMOOTH_CHANNEL_DTYPE) if name == "channels" else np.zeros((E, K), dtype=_DTYPES[name][1])
    rc = _lib.load().gat_smooth_observables_host(*[addr(a.get(n)) for n in _INPUTS + ("doppler_hz", "valid")], int(E), int(K), C.byref(cfg),
                                                 addr(raw["tx_frac_out"]), *[addr(raw.get(n)) for n in OUTPUTS])
    host_check(rc, "gat_smooth_observables_host")
    return SmoothedObservables(raw)


def smoothing_plan(num_epochs: int, num_channels: int, *, window: int = 100, cmc_gate_m: float = 15.0, rate_gate_cycles: float | None = None,
                   carrier_hz: float = 1575.42e6, if_hz: float = 0.0, epoch_seconds: float = 1e-3) -> dict:
    """``gat_smooth_observables_plan``: the chunk length and count, lanes, rows and run of a chunk's workgroup, the threads, LDS
    bytes and workgroups of the kernels and the scratch bytes of such a call."""
    cfg = smooth_config(window=window, if_hz=if_hz, epoch_seconds=epoch_seconds, cmc_gate_s=float(cmc_gate_m) / C_LIGHT,
                        rate_gate_cycles=rate_gate_cycles, carrier_hz=carrier_hz)
    plan = new_plan(_lib.SmoothPlan)
    rc = _lib.load().gat_smooth_observables_plan(int(num_epochs), int(num_channels), C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_smooth_observables_plan")
    return plan_report(plan)
