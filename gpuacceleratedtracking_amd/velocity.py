"""Velocity fix (include/gat.h, "velocity fix"): from the Doppler observable and a position fix to a velocity::

    obs = observables(...)                                        # gat_observables: tx_ms, tx_frac, doppler_hz [E, K]
    fix = position_fix(ephs, obs.tx_ms, obs.tx_frac, rx_ms, rx_frac)
    vel = velocity_fix(ephs, obs.tx_ms, obs.tx_frac, obs.doppler_hz, fix)    # gat_velocity_fix: enqueued, not synchronised
    vel.v_ecef, vel.v_enu, vel.speed, vel.clock_drift, vel.status           # per epoch
    vel.lat_deg, vel.lon_deg, vel.height_m                                  # the geodetic frame the velocity was turned into
    vel.sat_vel, vel.resid                                                  # per epoch and channel

The work is libgat's HIP kernel (``velocity_fix``) or its host twin with the same bits (``velocity_fix_host``).  A ``VelocityFix``
of the device call keeps device tensors and reads them back (after ``ctx.sync()``) at the first look at a value.  The library
gives the frame as sines and cosines; the angles in degrees are numpy's, outside the rule."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .positioning import PositionFix, ephemeris_records
from .results import PlannedResult, host_check, new_plan, plan_report, wanted
from .streams import addr, keep_alive, vp

FEW_SATS, SINGULAR, NONFINITE = _lib.GAT_VEL_FEW_SATS, _lib.GAT_VEL_SINGULAR, _lib.GAT_VEL_NONFINITE
NO_FIX, NO_GEODETIC = _lib.GAT_VEL_NO_FIX, _lib.GAT_VEL_NO_GEODETIC
OUTPUTS = ("sat_vel", "resid")
_SHAPES = {"sat_vel": (4,), "resid": ()}


def vel_config(carrier_hz: float = 1575.42e6, flags: int = 0) -> _lib.VelConfig:
    """``gat_vel_config`` from Python values.  Nothing is checked: the library refuses."""
    cfg = _lib.VelConfig()
    cfg.struct_size = C.sizeof(_lib.VelConfig)
    cfg.carrier_hz, cfg.flags = float(carrier_hz), int(flags)
    return cfg


class VelocityFix(PlannedResult):
    """The outputs of one call.  Raw: ``velocities`` (structured ``[E]``: status, num_valid, num_used, vx, vy, vz, clock_drift,
    rms_residual_mps, ve, vn, vu, sin_lat, cos_lat, sin_lon, cos_lon, height_m) and, where asked for, ``sat_vel`` ``[E, K, 4]`` (the
    satellites' ECEF velocity and clock rate) and ``resid`` ``[E, K]``.  Derived: every field of ``velocities`` ``[E]``, ``v_ecef``
    and ``v_enu`` ``[E, 3]``, ``speed``, ``lat_deg``, ``lon_deg`` and ``ok`` (status 0)."""

    _VIEWS = {"velocities": (_lib.VELOCITY_DTYPE, False)}

    def __getattr__(self, name):
        if name in _lib.VELOCITY_DTYPE.names:
            return self._h()["velocities"][name].copy()
        if name in OUTPUTS:
            if name not in self._raw:
                raise AttributeError(f"{name} was not asked for (outputs=)")
            return self._h()[name]
        raise AttributeError(name)

    velocities = property(lambda self: self._h()["velocities"])
    ok = property(lambda self: self.velocities["status"] == 0)

    @property
    def v_ecef(self) -> np.ndarray:
        v = self.velocities
        return np.stack([v["vx"], v["vy"], v["vz"]], axis=1)

    @property
    def v_enu(self) -> np.ndarray:
        v = self.velocities
        return np.stack([v["ve"], v["vn"], v["vu"]], axis=1)

    speed = property(lambda self: np.sqrt((self.v_ecef ** 2).sum(axis=1)), doc="float64 [E]: |v|, m/s")
    lat_deg = property(lambda self: np.degrees(np.arctan2(self.velocities["sin_lat"], self.velocities["cos_lat"])))
    lon_deg = property(lambda self: np.degrees(np.arctan2(self.velocities["sin_lon"], self.velocities["cos_lon"])))


def _fix_inputs(fix, used, host: bool):
    """the fix records and the used set of a call: a ``PositionFix`` gives its records (as the call left them, or read back for the
    host twin) and, for ``used="fix"``, its ``used`` output where it has one"""
    if isinstance(used, str) and used != "fix":
        raise ValueError('used must be "fix", None or a uint8 [E, K] array')
    if isinstance(fix, PositionFix):
        src = fix._h() if host else fix._raw
        records = src["fixes"]
        if isinstance(used, str):
            used = src.get("used")
    else:
        records = fix
        if isinstance(used, str):
            used = None
    return records, used


def velocity_fix(ephs, tx_ms, tx_frac, doppler_hz, fix, weights=None, *, used="fix", outputs=None, ctx: Context | None = None,
                 carrier_hz: float = 1575.42e6, flags: int = 0) -> VelocityFix:
    """``gat_velocity_fix`` on the device.  ``ephs``: ``Ephemeris`` objects (uploaded) or a uint8 device tensor of ``K`` records;
    ``tx_ms`` int32, ``tx_frac`` and ``doppler_hz`` float64 ``[E, K]``, ``weights`` float64 ``[E, K]`` or None: contiguous device
    tensors, passed as they are.  ``fix``: the ``PositionFix`` of ``position_fix`` / ``position_fix_raim`` or a uint8 device tensor
    of ``E`` ``gat_fix`` records.  ``used``: "fix" (the fix's own ``used`` output where it has one, else every channel), None
    (every channel) or a uint8 ``[E, K]`` device tensor.  ``outputs``: which of "sat_vel", "resid" to write (None: both).  Enqueues
    on the context's stream and returns at once."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    records, used = _fix_inputs(fix, used, host=False)
    for name, t, dt in (("tx_ms", tx_ms, torch.int32), ("tx_frac", tx_frac, torch.float64), ("doppler_hz", doppler_hz, torch.float64),
                        ("weights", weights, torch.float64), ("used", used, torch.uint8), ("fix", records, torch.uint8)):
        if t is None and name in ("weights", "used"):
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
        if not t.is_cuda or t.device != tx_ms.device:
            raise ValueError(f"{name} must live on the HIP device, the same one as tx_ms")
    if tx_ms.dim() != 2 or any(t is not None and t.shape != tx_ms.shape for t in (tx_frac, doppler_hz, weights, used)):
        raise ValueError("tx_ms, tx_frac, doppler_hz, weights and used must be [E, K]")
    E, K = (int(v) for v in tx_ms.shape)
    if records.numel() != E * _lib.FIX_DTYPE.itemsize:
        raise ValueError(f"fix must hold {E} gat_fix records")
    dev = tx_ms.device
    if isinstance(ephs, torch.Tensor):
        eph_dev = ephs
        if eph_dev.dtype != torch.uint8 or not eph_dev.is_contiguous() or eph_dev.numel() != K * _lib.EPHEMERIS_DTYPE.itemsize or eph_dev.device != dev:
            raise ValueError("ephs must be the K records as a contiguous uint8 tensor on the device of tx_ms")
    else:
        recs = ephemeris_records(ephs)
        if recs.shape[0] != K:
            raise ValueError(f"{recs.shape[0]} ephemerides for {K} channels")
        eph_dev = torch.from_numpy(recs.view(np.uint8).reshape(K, -1).copy()).to(dev)
    if ctx is None:
        ctx = get_context(dev)
    cfg = vel_config(carrier_hz, flags)
    raw = {"velocities": torch.empty((E, _lib.VELOCITY_DTYPE.itemsize), dtype=torch.uint8, device=dev)}
    for name in want:
        raw[name] = torch.empty((E, K) + _SHAPES[name], dtype=torch.float64, device=dev)
    ctx.check(ctx.lib.gat_velocity_fix(ctx._h, vp(eph_dev), vp(tx_ms), vp(tx_frac), vp(doppler_hz), vp(records), vp(used), vp(weights), E, K,
                                       C.byref(cfg), vp(raw["velocities"]), *[vp(raw.get(n)) for n in OUTPUTS]), "gat_velocity_fix")
    return keep_alive(VelocityFix(raw, ctx), eph_dev, tx_ms, tx_frac, doppler_hz, records, used, weights)


def velocity_fix_host(ephs, tx_ms, tx_frac, doppler_hz, fix, weights=None, *, used="fix", outputs=None, carrier_hz: float = 1575.42e6,
                      flags: int = 0) -> VelocityFix:
    """``gat_velocity_fix_host``: the same rule and the same bits over numpy arrays; needs no device.  ``fix``: a ``PositionFix``
    (of either call: it is read back) or a structured ``gat_fix`` array ``[E]``."""
    want = wanted(outputs, OUTPUTS, OUTPUTS)
    records, used = _fix_inputs(fix, used, host=True)
    recs = ephemeris_records(ephs)
    tx_ms = np.ascontiguousarray(tx_ms, dtype=np.int32)
    tx_frac, doppler_hz = np.ascontiguousarray(tx_frac, dtype=np.float64), np.ascontiguousarray(doppler_hz, dtype=np.float64)
    if tx_ms.ndim != 2 or tx_frac.shape != tx_ms.shape or doppler_hz.shape != tx_ms.shape:
        raise ValueError("tx_ms, tx_frac and doppler_hz must be [E, K]")
    E, K = (int(v) for v in tx_ms.shape)
    records = np.ascontiguousarray(records)
    if records.dtype != _lib.FIX_DTYPE or records.shape != (E,) or recs.shape[0] != K:
        raise ValueError("fix must be gat_fix records [E], and there must be K ephemerides")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
    if used is not None:
        used = np.ascontiguousarray(used, dtype=np.uint8)
    if any(a is not None and a.shape != tx_ms.shape for a in (weights, used)):
        raise ValueError("weights and used must be [E, K]")
    cfg = vel_config(carrier_hz, flags)
    raw = {"velocities": np.zeros(E, dtype=_lib.VELOCITY_DTYPE)}
    for name in want:
        raw[name] = np.zeros((E, K) + _SHAPES[name], dtype=np.float64)
    rc = _lib.load().gat_velocity_fix_host(addr(recs), addr(tx_ms), addr(tx_frac), addr(doppler_hz), addr(records), addr(used), addr(weights), E, K,
                                           C.byref(cfg), addr(raw["velocities"]), *[addr(raw.get(n)) for n in OUTPUTS])
    host_check(rc, "gat_velocity_fix_host")
    return VelocityFix(raw)


def velocity_plan(num_epochs: int, num_channels: int, *, carrier_hz: float = 1575.42e6, flags: int = 0) -> dict:
    """``gat_velocity_fix_plan``: ``position_plan``'s report for such a call."""
    cfg = vel_config(carrier_hz, flags)
    plan = new_plan(_lib.FixPlan)
    rc = _lib.load().gat_velocity_fix_plan(int(num_epochs), int(num_channels), C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_velocity_fix_plan")
    return plan_report(plan)
