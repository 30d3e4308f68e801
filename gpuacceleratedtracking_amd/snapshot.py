"""Snapshot fix (include/gat.h, "snapshot fix"): a coarse-time position from code phases alone, without bit sync, frame sync or a
decoded time of week::

    res = acquire(GPSL1, signal, fs, prns, method="fft")                  # a few milliseconds of samples
    prns, frac = code_fractions(res, GPSL1)                               # the transmit times modulo 1 ms
    snap = snapshot_fix(ephs, frac[None], rx_ms, rx_frac, prior_xyz)      # gat_snapshot_fix: enqueued, not synchronised
    snap.xyz, snap.clock_bias_s, snap.coarse_time_s, snap.status          # per epoch
    position_fix_raim(ephs, snap.raw("tx_ms"), frac[None], snap.raw("rx_ms_out"), rx_frac, ...)   # nothing read back in between

The work is libgat's HIP kernel (``snapshot_fix``) or its host twin with the same bits (``snapshot_fix_host``).  A ``SnapshotFix``
of the device call keeps device tensors and reads them back (after ``ctx.sync()``) at the first look at a value; ``raw(name)``
gives an output as the call left it (a device tensor, or a numpy array of the twin) for the next call."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .positioning import ephemeris_records
from .results import PlannedResult, host_check, new_plan, plan_report, wanted
from .signals import get_code_frequency, get_code_length
from .streams import addr, keep_alive, vp

FEW_SATS, SINGULAR, NONFINITE, NOT_CONVERGED = _lib.GAT_SNAP_FEW_SATS, _lib.GAT_SNAP_SINGULAR, _lib.GAT_SNAP_NONFINITE, _lib.GAT_SNAP_NOT_CONVERGED
MASK_STARVED, MASKED, AMBIGUOUS, RERESOLVED = _lib.GAT_SNAP_MASK_STARVED, _lib.GAT_SNAP_MASKED, _lib.GAT_SNAP_AMBIGUOUS, _lib.GAT_SNAP_RERESOLVED
OUTPUTS = ("tx_ms", "rx_ms_out", "n_ms", "resid", "sin_el", "used")
_TORCH = {"tx_ms": torch.int32, "rx_ms_out": torch.int32, "n_ms": torch.int32, "resid": torch.float64, "sin_el": torch.float64, "used": torch.uint8}
_NUMPY = {"tx_ms": np.int32, "rx_ms_out": np.int32, "n_ms": np.int32, "resid": np.float64, "sin_el": np.float64, "used": np.uint8}


def snap_config(max_iter: int = 10, tol_m: float = 1e-4, mask_sin: float = -1.0, init_xyz=(0.0, 0.0, 0.0), ambiguity_margin: float = 0.1,
                flags: int = 0) -> _lib.SnapConfig:
    """``gat_snap_config`` from Python values.  Nothing is checked: the library refuses."""
    cfg = _lib.SnapConfig()
    cfg.struct_size = C.sizeof(_lib.SnapConfig)
    cfg.max_iter, cfg.tol_m, cfg.mask_sin, cfg.flags = int(max_iter), float(tol_m), float(mask_sin), int(flags)
    cfg.ambiguity_margin = float(ambiguity_margin)
    for i in range(3):
        cfg.init_xyz[i] = float(init_xyz[i])
    return cfg


def code_fractions(results, system) -> tuple[np.ndarray, np.ndarray]:
    """A list of ``AcquisitionResult`` as the snapshot fix's measurement: (``prns`` int32 ``[K]``, 0-based as the results carry them,
    ``code_frac`` float64 ``[K]``: the code phase at the block's first sample over the chipping rate, the transmit time modulo one
    code period).  A result that was not detected gives NaN: no measurement."""
    fc, length = float(get_code_frequency(system)), float(get_code_length(system))
    prns = np.array([r.prn for r in results], dtype=np.int32)
    frac = np.array([(float(r.code_phase) % length) / fc if r.detected == 1 else np.nan for r in results], dtype=np.float64)
    frac[frac >= length / fc] = 0.0  # a phase that rounds up to the whole period
    return prns, frac


class SnapshotFix(PlannedResult):
    """The outputs of one call.  Raw: ``fixes`` (structured ``[E]``: status, num_valid, num_used, iterations, x, y, z, clock_bias_s,
    coarse_time_s, rms_residual_m, last_step_m, gdop, pdop, tdop) and, where asked for, ``tx_ms`` and ``n_ms`` int32 ``[E, K]``,
    ``rx_ms_out`` int32 ``[E]``, ``resid`` and ``sin_el`` ``[E, K]``, ``used`` uint8 ``[E, K]``.  Derived: every field of ``fixes``
    ``[E]``, ``xyz`` ``[E, 3]`` and ``ok`` (status 0)."""

    _VIEWS = {"fixes": (_lib.SNAP_FIX_DTYPE, False)}

    def __getattr__(self, name):
        if name in _lib.SNAP_FIX_DTYPE.names:
            return self._h()["fixes"][name].copy()
        if name in OUTPUTS:
            if name not in self._raw:
                raise AttributeError(f"{name} was not asked for (outputs=)")
            return self._h()[name]
        raise AttributeError(name)

    fixes = property(lambda self: self._h()["fixes"])
    ok = property(lambda self: self.fixes["status"] == 0)

    @property
    def xyz(self) -> np.ndarray:
        f = self.fixes
        return np.stack([f["x"], f["y"], f["z"]], axis=1)

    def raw(self, name: str):
        """an output as the call left it: a device tensor of ``snapshot_fix`` (nothing is read back), a numpy array of the twin"""
        if name not in self._raw:
            raise AttributeError(f"{name} was not asked for (outputs=)")
        return self._raw[name]


def _shape(name: str, E: int, K: int) -> tuple:
    return (E,) if name == "rx_ms_out" else (E, K)


def snapshot_fix(ephs, code_frac, rx_ms, rx_frac, prior_xyz=None, weights=None, *, outputs=None, ctx: Context | None = None,
                 **config) -> SnapshotFix:
    """``gat_snapshot_fix`` on the device.  ``ephs``: ``Ephemeris`` objects (uploaded) or a uint8 device tensor of ``K`` records;
    ``code_frac`` float64 ``[E, K]``, ``rx_ms`` int32 and ``rx_frac`` float64 ``[E]``, ``prior_xyz`` float64 ``[E, 3]`` or None (then
    ``init_xyz`` of the config), ``weights`` float64 ``[E, K]`` or None: contiguous device tensors, passed as they are.
    ``outputs``: which of "tx_ms", "rx_ms_out", "n_ms", "resid", "sin_el", "used" to write (None: all).  ``config``: ``max_iter``,
    ``tol_m``, ``mask_sin``, ``init_xyz``, ``ambiguity_margin``.  Enqueues on the context's stream and returns at once."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    for name, t, dt in (("code_frac", code_frac, torch.float64), ("rx_ms", rx_ms, torch.int32), ("rx_frac", rx_frac, torch.float64),
                        ("prior_xyz", prior_xyz, torch.float64), ("weights", weights, torch.float64)):
        if t is None and name in ("prior_xyz", "weights"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
        if not t.is_cuda or t.device != code_frac.device:
            raise ValueError(f"{name} must live on the HIP device, the same one as code_frac")
    if code_frac.dim() != 2 or (weights is not None and weights.shape != code_frac.shape):
        raise ValueError("code_frac and weights must be [E, K]")
    E, K = (int(v) for v in code_frac.shape)
    if rx_ms.shape != (E,) or rx_frac.shape != (E,) or (prior_xyz is not None and prior_xyz.shape != (E, 3)):
        raise ValueError("rx_ms and rx_frac must be [E], prior_xyz [E, 3]")
    dev = code_frac.device
    if isinstance(ephs, torch.Tensor):
        eph_dev = ephs
        if eph_dev.dtype != torch.uint8 or not eph_dev.is_contiguous() or eph_dev.numel() != K * _lib.EPHEMERIS_DTYPE.itemsize or eph_dev.device != dev:
            raise ValueError("ephs must be the K records as a contiguous uint8 tensor on the device of code_frac")
    else:
        recs = ephemeris_records(ephs)
        if recs.shape[0] != K:
            raise ValueError(f"{recs.shape[0]} ephemerides for {K} channels")
        eph_dev = torch.from_numpy(recs.view(np.uint8).reshape(K, -1).copy()).to(dev)
    if ctx is None:
        ctx = get_context(dev)
    cfg = snap_config(**config)
    raw = {"fixes": torch.empty((E, _lib.SNAP_FIX_DTYPE.itemsize), dtype=torch.uint8, device=dev)}
    for name in want:
        raw[name] = torch.empty(_shape(name, E, K), dtype=_TORCH[name], device=dev)
    ctx.check(ctx.lib.gat_snapshot_fix(ctx._h, vp(eph_dev), vp(code_frac), vp(rx_ms), vp(rx_frac), vp(prior_xyz), vp(weights), E, K, C.byref(cfg),
                                       vp(raw["fixes"]), *[vp(raw.get(n)) for n in OUTPUTS]), "gat_snapshot_fix")
    return keep_alive(SnapshotFix(raw, ctx), eph_dev, code_frac, rx_ms, rx_frac, prior_xyz, weights)


def snapshot_fix_host(ephs, code_frac, rx_ms, rx_frac, prior_xyz=None, weights=None, *, outputs=None, **config) -> SnapshotFix:
    """``gat_snapshot_fix_host``: the same rule and the same bits over numpy arrays; needs no device."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    recs = ephemeris_records(ephs)
    code_frac = np.ascontiguousarray(code_frac, dtype=np.float64)
    rx_ms, rx_frac = np.ascontiguousarray(rx_ms, dtype=np.int32), np.ascontiguousarray(rx_frac, dtype=np.float64)
    if code_frac.ndim != 2:
        raise ValueError("code_frac must be [E, K]")
    E, K = (int(v) for v in code_frac.shape)
    if rx_ms.shape != (E,) or rx_frac.shape != (E,) or recs.shape[0] != K:
        raise ValueError("rx_ms and rx_frac must be [E], and there must be K ephemerides")
    if prior_xyz is not None:
        prior_xyz = np.ascontiguousarray(prior_xyz, dtype=np.float64)
        if prior_xyz.shape != (E, 3):
            raise ValueError("prior_xyz must be [E, 3]")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != code_frac.shape:
            raise ValueError("weights must be [E, K]")
    cfg = snap_config(**config)
    raw = {"fixes": np.zeros(E, dtype=_lib.SNAP_FIX_DTYPE)}
    for name in want:
        raw[name] = np.zeros(_shape(name, E, K), dtype=_NUMPY[name])
    rc = _lib.load().gat_snapshot_fix_host(addr(recs), addr(code_frac), addr(rx_ms), addr(rx_frac), addr(prior_xyz), addr(weights), E, K,
                                           C.byref(cfg), addr(raw["fixes"]), *[addr(raw.get(n)) for n in OUTPUTS])
    host_check(rc, "gat_snapshot_fix_host")
    return SnapshotFix(raw)


def snapshot_plan(num_epochs: int, num_channels: int, **config) -> dict:
    """``gat_snapshot_fix_plan``: ``position_plan``'s report for such a call (the LDS is the snapshot fix's own: 20 terms)."""
    cfg = snap_config(**config)
    plan = new_plan(_lib.FixPlan)
    rc = _lib.load().gat_snapshot_fix_plan(int(num_epochs), int(num_channels), C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_snapshot_fix_plan")
    return plan_report(plan)
