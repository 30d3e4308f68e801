"""Position fix (include/gat.h, "position fix"): from the decoder's checked words and the observables to a position::

    nav = loop.navigation(mon)                                   # gat_nav_decode: subframes 1 - 3 of every channel
    ephs = lnav_ephemerides(nav)                                 # gat_lnav_ephemeris_host: one Ephemeris a channel
    fix = position_fix(ephs, tx_ms, tx_frac, rx_ms, rx_frac)     # gat_position_fix: enqueued, not synchronised
    fix.xyz, fix.clock_bias_s, fix.status, fix.pdop              # per epoch
    fix.sat, fix.resid, fix.sin_el, fix.used                     # per epoch and channel
    fix = position_fix_raim(ephs, tx_ms, tx_frac, rx_ms, rx_frac, sigma_m=3.0)   # gat_position_fix_raim: the fix with integrity
    fix.detected, fix.excluded, fix.integrity                    # per epoch: the residual test and the channels left out

A time of the week is whole milliseconds (int32) and a fraction in seconds (float64): ``tx_ms``, ``tx_frac`` ``[E, K]`` of
transmission, ``rx_ms``, ``rx_frac`` ``[E]`` of reception.  The work is libgat's HIP kernel (``position_fix``) or its host twin with
the same bits (``position_fix_host``).  A ``PositionFix`` of the device call keeps device tensors and reads them back (after
``ctx.sync()``) at the first look at a value.  ``lnav_ephemeris_payloads`` is the encoder a simulation needs: the payload bits of
subframes 1 - 3 in the form ``lnav_subframe(payload=)`` takes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .navigation import NavResult
from .results import PlannedResult, host_check, new_plan, plan_report, wanted
from .streams import addr, keep_alive, vp

FEW_SATS, SINGULAR, NONFINITE = _lib.GAT_FIX_FEW_SATS, _lib.GAT_FIX_SINGULAR, _lib.GAT_FIX_NONFINITE
NOT_CONVERGED, MASK_STARVED, MASKED = _lib.GAT_FIX_NOT_CONVERGED, _lib.GAT_FIX_MASK_STARVED, _lib.GAT_FIX_MASKED
OUTPUTS = ("sat", "resid", "sin_el", "used")
EXCLUDED = _lib.GAT_FIX_EXCLUDED  # in ``status``, by position_fix_raim alone
RAIM_NOT_CHECKED, RAIM_NO_REDUNDANCY, RAIM_DETECTED = _lib.GAT_RAIM_NOT_CHECKED, _lib.GAT_RAIM_NO_REDUNDANCY, _lib.GAT_RAIM_DETECTED
RAIM_EXCLUDED, RAIM_UNRESOLVED = _lib.GAT_RAIM_EXCLUDED, _lib.GAT_RAIM_UNRESOLVED
RAIM_OUTPUTS = OUTPUTS + ("trial",)


class Ephemeris:
    """``gat_ephemeris``: SI units and radians.  Integers ``wn, iodc, iode, health, ura, fit``; floats ``toc, toe, af0, af1, af2, tgd,
    sqrt_a, e, m0, delta_n, omega0, i0, omega, omega_dot, idot, cuc, cus, crc, crs, cic, cis``; ``valid`` and ``reason`` (why not)."""

    FIELDS = _lib.EPHEMERIS_DTYPE.names

    def __init__(self, **fields):
        unknown = set(fields) - set(self.FIELDS)
        if unknown:
            raise TypeError(f"unknown ephemeris fields {sorted(unknown)}")
        self.record = np.zeros((), dtype=_lib.EPHEMERIS_DTYPE)
        self.record["valid"] = 1
        for name, value in fields.items():
            self.record[name] = value

    @classmethod
    def from_record(cls, record) -> "Ephemeris":
        eph = cls()
        eph.record = np.array(record, dtype=_lib.EPHEMERIS_DTYPE).reshape(())
        return eph

    def __getattr__(self, name):
        if name in type(self).FIELDS:
            return self.__dict__["record"][name].item()
        raise AttributeError(name)

    def __eq__(self, other):
        return isinstance(other, Ephemeris) and self.record.tobytes() == other.record.tobytes()

    def __repr__(self):
        return "Ephemeris(" + ", ".join(f"{n}={self.record[n].item()!r}" for n in self.FIELDS) + ")"


def ephemeris_records(ephs) -> np.ndarray:
    """``gat_ephemeris [K]`` as a structured array from a sequence of ``Ephemeris`` (or such an array)"""
    if isinstance(ephs, np.ndarray) and ephs.dtype == _lib.EPHEMERIS_DTYPE:
        return np.ascontiguousarray(ephs.reshape(-1))
    if isinstance(ephs, Ephemeris):
        ephs = [ephs]
    return np.array([e.record for e in ephs], dtype=_lib.EPHEMERIS_DTYPE).reshape(-1)


def lnav_ephemeris(nav: NavResult, channel: int) -> Ephemeris:
    """``gat_lnav_ephemeris_host`` on one channel's frames: the newest complete set of good subframes 1, 2 and 3 of one issue.
    ``valid`` is 0 where there are none (``reason``: ``GAT_EPH_MISSING`` / ``GAT_EPH_IODE``)."""
    frames = np.ascontiguousarray(nav.frames[int(channel)])
    rec = np.zeros((), dtype=_lib.EPHEMERIS_DTYPE)
    rc = _lib.load().gat_lnav_ephemeris_host(addr(frames), int(frames.shape[0]), addr(rec))
    host_check(rc, "gat_lnav_ephemeris_host")
    return Ephemeris.from_record(rec)


def lnav_ephemerides(nav: NavResult) -> list:
    """``lnav_ephemeris`` of every channel of the decoder's result"""
    return [lnav_ephemeris(nav, k) for k in range(nav.frames.shape[0])]


def lnav_ephemeris_payloads(eph: Ephemeris) -> np.ndarray:
    """``gat_lnav_ephemeris_words_host``: uint8 ``[3, 190]``, the quantised payload bits of subframes 1, 2 and 3 -- row ``i`` is what
    ``lnav_subframe(tow, i + 1, payload=)`` takes."""
    bits = np.zeros((3, 190), dtype=np.uint8)
    rec = np.ascontiguousarray(eph.record)
    rc = _lib.load().gat_lnav_ephemeris_words_host(addr(rec), addr(bits))
    host_check(rc, "gat_lnav_ephemeris_words_host")
    return bits


def fix_config(max_iter: int = 10, tol_m: float = 1e-4, mask_sin: float = -1.0, init_xyz=(0.0, 0.0, 0.0), flags: int = 0) -> _lib.FixConfig:
    """``gat_fix_config`` from Python values.  Nothing is checked: the library refuses."""
    cfg = _lib.FixConfig()
    cfg.struct_size = C.sizeof(_lib.FixConfig)
    cfg.max_iter, cfg.tol_m, cfg.mask_sin, cfg.flags = int(max_iter), float(tol_m), float(mask_sin), int(flags)
    for i in range(3):
        cfg.init_xyz[i] = float(init_xyz[i])
    return cfg


class PositionFix(PlannedResult):
    """The outputs of one call.  Raw: ``fixes`` (structured ``[E]``: status, num_valid, num_used, iterations, x, y, z, clock_bias_s,
    rms_residual_m, last_step_m, gdop, pdop) and, where asked for, ``sat`` ``[E, K, 4]`` (ECEF at transmission and the clock
    correction), ``resid`` and ``sin_el`` ``[E, K]``, ``used`` uint8 ``[E, K]``.  Derived: every field of ``fixes`` ``[E]``, ``xyz``
    ``[E, 3]`` and ``ok`` (status 0).  Of ``position_fix_raim``: ``integrity`` (structured ``[E]``), ``excluded`` ``[E, 4]``,
    ``detected`` ``[E]`` and, where asked for, ``trial`` ``[E, K]``."""

    _VIEWS = {"fixes": (_lib.FIX_DTYPE, False), "integrity": (_lib.INTEGRITY_DTYPE, False)}

    def __getattr__(self, name):
        if name in _lib.FIX_DTYPE.names:
            return self._h()["fixes"][name].copy()
        if name in RAIM_OUTPUTS:
            if name not in self._raw:
                raise AttributeError(f"{name} was not asked for (outputs=)")
            return self._h()[name]
        raise AttributeError(name)

    fixes = property(lambda self: self._h()["fixes"])
    ok = property(lambda self: self.fixes["status"] == 0)

    # of position_fix_raim alone
    @property
    def integrity(self) -> np.ndarray:
        """``gat_fix_integrity`` structured ``[E]``: status (``RAIM_*`` bits), dof, num_excluded, excluded ``[4]``, stat0, threshold0,
        stat, threshold"""
        if "integrity" not in self._raw:
            raise AttributeError("integrity: not a result of position_fix_raim")
        return self._h()["integrity"]

    excluded = property(lambda self: self.integrity["excluded"].copy(), doc="int32 [E, 4]: the channels left out, in order; -1 where unused")
    detected = property(lambda self: (self.integrity["status"] & RAIM_DETECTED) != 0, doc="bool [E]: the full set failed the test")

    @property
    def xyz(self) -> np.ndarray:
        f = self.fixes
        return np.stack([f["x"], f["y"], f["z"]], axis=1)


_SHAPES = {"sat": (4,), "resid": (), "sin_el": (), "used": (), "trial": ()}


def _device_args(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights):
    """the checks of a device call: (E, K, the device, the ephemerides on it)"""
    for name, t, dt in (("tx_ms", tx_ms, torch.int32), ("tx_frac", tx_frac, torch.float64), ("rx_ms", rx_ms, torch.int32),
                        ("rx_frac", rx_frac, torch.float64), ("weights", weights, torch.float64)):
        if t is None and name == "weights":
            continue
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous {dt} device tensor")
        if not t.is_cuda or t.device != tx_ms.device:
            raise ValueError(f"{name} must live on the HIP device, the same one as tx_ms")
    if tx_ms.dim() != 2 or tx_frac.shape != tx_ms.shape or (weights is not None and weights.shape != tx_ms.shape):
        raise ValueError("tx_ms, tx_frac and weights must be [E, K]")
    E, K = (int(v) for v in tx_ms.shape)
    if rx_ms.shape != (E,) or rx_frac.shape != (E,):
        raise ValueError("rx_ms and rx_frac must be [E]")
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
    return E, K, dev, eph_dev


def _device_fix(raim, ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs, ctx, config) -> PositionFix:
    """the device call of both: ``raim`` None is ``gat_position_fix``, else ``_raim_setup``'s arguments after the weights"""
    want = wanted(outputs, OUTPUTS if raim is None else RAIM_OUTPUTS, OUTPUTS)
    E, K, dev, eph_dev = _device_args(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights)
    if ctx is None:
        ctx = get_context(dev)
    cfg = fix_config(**config)
    raw = {"fixes": torch.empty((E, _lib.FIX_DTYPE.itemsize), dtype=torch.uint8, device=dev)}
    for name in want:
        raw[name] = torch.empty((E, K) + _SHAPES[name], dtype=torch.uint8 if name == "used" else torch.float64, device=dev)
    call = (ctx._h, vp(eph_dev), vp(tx_ms), vp(tx_frac), vp(rx_ms), vp(rx_frac), vp(weights), E, K, C.byref(cfg))
    outs = [vp(raw.get(n)) for n in OUTPUTS]
    if raim is None:
        ctx.check(ctx.lib.gat_position_fix(*call, vp(raw["fixes"]), *outs), "gat_position_fix")
    else:
        rcfg = _raim_setup(weights, *raim)
        raw["integrity"] = torch.empty((E, _lib.INTEGRITY_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        ctx.check(ctx.lib.gat_position_fix_raim(*call, C.byref(rcfg), vp(raw["fixes"]), vp(raw["integrity"]), *outs, vp(raw.get("trial"))),
                  "gat_position_fix_raim")
    return keep_alive(PositionFix(raw, ctx), eph_dev, tx_ms, tx_frac, rx_ms, rx_frac, weights)


def _host_fix(raim, ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs, config) -> PositionFix:
    """the host twin of both, as ``_device_fix``"""
    want = wanted(outputs, OUTPUTS if raim is None else RAIM_OUTPUTS, OUTPUTS)
    recs, tx_ms, tx_frac, rx_ms, rx_frac, weights, E, K = _host_args(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights)
    cfg = fix_config(**config)
    raw = {"fixes": np.zeros(E, dtype=_lib.FIX_DTYPE)}
    for name in want:
        raw[name] = np.zeros((E, K) + _SHAPES[name], dtype=np.uint8 if name == "used" else np.float64)
    call = (addr(recs), addr(tx_ms), addr(tx_frac), addr(rx_ms), addr(rx_frac), addr(weights), E, K, C.byref(cfg))
    outs = [addr(raw.get(n)) for n in OUTPUTS]
    if raim is None:
        host_check(_lib.load().gat_position_fix_host(*call, addr(raw["fixes"]), *outs), "gat_position_fix_host")
    else:
        rcfg = _raim_setup(weights, *raim)
        raw["integrity"] = np.zeros(E, dtype=_lib.INTEGRITY_DTYPE)
        host_check(_lib.load().gat_position_fix_raim_host(*call, C.byref(rcfg), addr(raw["fixes"]), addr(raw["integrity"]), *outs,
                                                          addr(raw.get("trial"))), "gat_position_fix_raim_host")
    return PositionFix(raw)


def position_fix(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights=None, *, outputs=None, ctx: Context | None = None, **config) -> PositionFix:
    """``gat_position_fix`` on the device.  ``ephs``: ``Ephemeris`` objects (uploaded) or a uint8 device tensor of ``K`` records;
    ``tx_ms`` int32 and ``tx_frac`` float64 ``[E, K]``, ``rx_ms`` int32 and ``rx_frac`` float64 ``[E]``, ``weights`` float64 ``[E, K]``
    or None: contiguous device tensors, passed as they are.  ``outputs``: which of "sat", "resid", "sin_el", "used" to write (None:
    all).  ``config``: ``max_iter``, ``tol_m``, ``mask_sin``, ``init_xyz``.  Enqueues on the context's stream and returns at once."""
    return _device_fix(None, ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs, ctx, config)


def position_fix_host(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights=None, *, outputs=None, **config) -> PositionFix:
    """``gat_position_fix_host``: the same rule and the same bits over numpy arrays; needs no device."""
    return _host_fix(None, ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs, config)


def _host_args(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights):
    """the checks of a host call: the arrays as the library takes them, E and K"""
    recs = ephemeris_records(ephs)
    tx_ms, rx_ms = np.ascontiguousarray(tx_ms, dtype=np.int32), np.ascontiguousarray(rx_ms, dtype=np.int32)
    tx_frac, rx_frac = np.ascontiguousarray(tx_frac, dtype=np.float64), np.ascontiguousarray(rx_frac, dtype=np.float64)
    if tx_ms.ndim != 2 or tx_frac.shape != tx_ms.shape:
        raise ValueError("tx_ms and tx_frac must be [E, K]")
    E, K = tx_ms.shape
    if rx_ms.shape != (E,) or rx_frac.shape != (E,) or recs.shape[0] != K:
        raise ValueError("rx_ms and rx_frac must be [E], and there must be K ephemerides")
    if weights is not None:
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if weights.shape != tx_ms.shape:
            raise ValueError("weights must be [E, K]")
    return recs, tx_ms, tx_frac, rx_ms, rx_frac, weights, int(E), int(K)


def position_plan(num_epochs: int, num_channels: int, **config) -> dict:
    """``gat_position_fix_plan``: the workgroups, the waves (epochs) of each, its threads and LDS, and the scratch bytes of such a call."""
    cfg = fix_config(**config)
    plan = new_plan(_lib.FixPlan)
    rc = _lib.load().gat_position_fix_plan(int(num_epochs), int(num_channels), C.byref(cfg), C.byref(plan))
    host_check(rc, "gat_position_fix_plan")
    return plan_report(plan)


# ---- fix integrity (include/gat.h, "fix integrity") -------------------------------------------------------------------------------
def _gamma_q(a: float, x: float) -> float:
    """the regularised upper incomplete gamma function Q(a, x): the series of P below a + 1, Lentz's continued fraction above"""
    import math

    if x <= 0.0:
        return 1.0
    lead = math.exp(a * math.log(x) - x - math.lgamma(a))
    if x < a + 1.0:
        term = total = 1.0 / a
        n = a
        while abs(term) > abs(total) * 1e-17:
            n += 1.0
            term *= x / n
            total += term
        return 1.0 - lead * total
    tiny = 1e-300
    b = x + 1.0 - a
    c, d = 1.0 / tiny, 1.0 / b
    h = d
    for i in range(1, 10000):
        an = -i * (i - a)
        b += 2.0
        d = an * d + b
        d = tiny if abs(d) < tiny else d
        c = b + an / c
        c = tiny if abs(c) < tiny else c
        d = 1.0 / d
        delta = d * c
        h *= delta
        if abs(delta - 1.0) < 1e-16:
            break
    return lead * h


def chi2_quantile(p_fa: float, dof: int) -> float:
    """the value a chi-square variable of ``dof`` degrees of freedom exceeds with probability ``p_fa``: Q(dof / 2, x / 2) = p_fa by
    bisection"""
    if not 0.0 < p_fa < 1.0 or dof < 1:
        raise ValueError("p_fa must lie in (0, 1) and dof be positive")
    a = 0.5 * dof
    lo, hi = 0.0, max(1.0, a)
    while _gamma_q(a, hi) > p_fa:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if _gamma_q(a, mid) > p_fa:
            lo = mid
        else:
            hi = mid
    return 2.0 * 0.5 * (lo + hi)


def raim_thresholds(p_fa: float = 1e-3, sigma_m: float = 1.0) -> np.ndarray:
    """float64 ``[GAT_MAX_FIX_CHANNELS - 3]``, by d = n - 4: ``sigma_m``^2 times the chi-square quantile at 1 - ``p_fa`` of d degrees of
    freedom, d = 1 .. 60 -- what T = sum w v^2 stays under with probability 1 - p_fa when the pseudorange errors are independent
    with standard deviation ``sigma_m`` (unit weights) or 1 / sqrt(w) (``sigma_m`` = 1).  Entry 0 is not read (0)."""
    out = np.zeros(_lib.GAT_MAX_FIX_CHANNELS - 3, dtype=np.float64)
    for d in range(1, out.shape[0]):
        out[d] = float(sigma_m) ** 2 * chi2_quantile(float(p_fa), d)
    return out


def raim_config(thresholds, max_exclude: int = 1, trial_iter: int = 8, flags: int = 0) -> _lib.RaimConfig:
    """``gat_raim_config`` from Python values.  Nothing is checked but the thresholds' count: the library refuses."""
    thresholds = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if thresholds.shape[0] != _lib.GAT_MAX_FIX_CHANNELS - 3:
        raise ValueError(f"thresholds must be [{_lib.GAT_MAX_FIX_CHANNELS - 3}], indexed by d = n - 4")
    cfg = _lib.RaimConfig()
    cfg.struct_size = C.sizeof(_lib.RaimConfig)
    cfg.max_exclude, cfg.trial_iter, cfg.flags = int(max_exclude), int(trial_iter), int(flags)
    for d, v in enumerate(thresholds):
        cfg.threshold[d] = float(v)
    return cfg


def _raim_setup(weights, thresholds, p_fa, sigma_m, max_exclude, trial_iter, raim_flags):
    if thresholds is None:
        if weights is None and sigma_m is None:
            raise ValueError("without weights the thresholds need sigma_m, the standard deviation of a pseudorange in metres")
        thresholds = raim_thresholds(p_fa, 1.0 if sigma_m is None else sigma_m)
    return raim_config(thresholds, max_exclude, trial_iter, raim_flags)


def position_fix_raim(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights=None, *, thresholds=None, p_fa: float = 1e-3, sigma_m=None,
                      max_exclude: int = 1, trial_iter: int = 8, raim_flags: int = 0, outputs=None, ctx: Context | None = None,
                      **config) -> PositionFix:
    """``gat_position_fix_raim`` on the device: ``position_fix`` with the residual test and fault exclusion.  The arguments are
    ``position_fix``'s; ``thresholds`` float64 ``[61]`` by d = n - 4 in the units of sum w v^2 (None: ``raim_thresholds(p_fa,
    sigma_m)`` -- with ``weights`` = 1 / sigma^2 leave ``sigma_m`` unset, without weights it is required), ``max_exclude`` rounds of
    exclusion (0: detect only), ``trial_iter`` iterations a leave-one-out trial.  ``outputs`` may also name "trial" (None: the fix's
    four).  The result also has ``integrity``, ``excluded``, ``detected`` and, where asked for, ``trial``."""
    return _device_fix((thresholds, p_fa, sigma_m, max_exclude, trial_iter, raim_flags), ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs, ctx,
                       config)


def position_fix_raim_host(ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights=None, *, thresholds=None, p_fa: float = 1e-3, sigma_m=None,
                           max_exclude: int = 1, trial_iter: int = 8, raim_flags: int = 0, outputs=None, **config) -> PositionFix:
    """``gat_position_fix_raim_host``: the same rule and the same bits over numpy arrays; needs no device."""
    return _host_fix((thresholds, p_fa, sigma_m, max_exclude, trial_iter, raim_flags), ephs, tx_ms, tx_frac, rx_ms, rx_frac, weights, outputs, config)


def raim_plan(num_epochs: int, num_channels: int, *, thresholds=None, p_fa: float = 1e-3, sigma_m: float = 1.0, max_exclude: int = 1,
              trial_iter: int = 8, raim_flags: int = 0, **config) -> dict:
    """``gat_position_fix_raim_plan``: ``position_plan``'s report for such a call (the LDS holds a round's frozen channels too)."""
    cfg = fix_config(**config)
    rcfg = _raim_setup(None, thresholds, p_fa, sigma_m, max_exclude, trial_iter, raim_flags)
    plan = new_plan(_lib.FixPlan)
    rc = _lib.load().gat_position_fix_raim_plan(int(num_epochs), int(num_channels), C.byref(cfg), C.byref(rcfg), C.byref(plan))
    host_check(rc, "gat_position_fix_raim_plan")
    return plan_report(plan)
