"""What the Python layer knows about the result and the plan of a planned call, stated once: the result object that keeps what
the call wrote and reads it back at the first look, the choice of optional outputs, how a ``gat_*_plan`` struct is made and
reported, and the refusal of a call that has no context.  The back-end modules (``monitor``, ``navigation``, ``observables``,
``positioning``) and the plan functions build on this one; it depends on ``_lib`` alone."""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib


class PlannedResult:
    """What one planned call wrote.  ``_raw``: its outputs by name, as the call left them (device tensors of a device call, numpy
    arrays of a host twin); ``_ctx``: the context of a device call, None for a host twin.  ``_VIEWS`` names the record buffers among
    them: ``name -> (structured dtype, rows)``, ``rows`` True for one row of records per channel, False for a flat array."""

    _VIEWS: dict = {}

    def __init__(self, raw: dict, ctx=None):
        self._raw, self._host, self._ctx = raw, None, ctx

    def _h(self) -> dict:
        """every output on the host: synchronises the context once, reads every tensor back once, views the record buffers"""
        if self._host is None:
            if self._ctx is not None:
                self._ctx.sync()
            host = {}
            for name, v in self._raw.items():
                a = v.cpu().numpy() if isinstance(v, torch.Tensor) else v
                if name in self._VIEWS:
                    dtype, rows = self._VIEWS[name]
                    a = a.view(dtype).reshape((a.shape[0], -1) if rows else -1)
                host[name] = a
            self._host = host
        return self._host


def wanted(outputs, known: tuple, default: tuple) -> tuple:
    """the optional outputs a call writes: ``default`` for None, else ``outputs``, every one of which must be among ``known``"""
    outputs = default if outputs is None else tuple(outputs)
    unknown = set(outputs) - set(known)
    if unknown:
        raise ValueError(f"unknown outputs {sorted(unknown)}: choose from {known}")
    return outputs


def new_plan(struct_cls):
    """a ``gat_*_plan`` struct for the library to fill: zeroed, ``struct_size`` set"""
    plan = struct_cls()
    plan.struct_size = C.sizeof(struct_cls)
    return plan


def plan_report(plan) -> dict:
    """the plan's fields as ints, without ``struct_size`` and ``reserved``"""
    return {n: int(getattr(plan, n)) for n, _ in plan._fields_ if n not in ("struct_size", "reserved")}


def host_check(rc: int, name: str) -> None:
    """the refusal of a call that has no context (a host twin, a plan): its code and the entry point's name"""
    if rc != 0:
        raise _lib.GatError(rc, name)
