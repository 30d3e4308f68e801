"""Closed tracking loop around the correlator: the layer Tracking.jl's
``track`` provides and the reference only touches to borrow buffers (``TrackingState``,
src/benchmarks.jl:54-61).  One ``TrackingLoop.step`` = one fused correlate launch for K channels
on one integration block + one ``gat_tracking_update`` launch that turns the accumulators into
the next block's parameters ON THE DEVICE (ping-pong parameter buffers, no host round trip).  With beamformer
weights (``TrackingLoop(weights=w)``, ``array.beamformer_weights``) the update forms prompt, early and late as
``sum_m conj(w[k, m]) R[m, tap]`` instead of the plain sum over antennas."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from .context import Context, get_context
from .gen_signal import make_params
from .results import host_check
from .signals import GNSSSystem, get_code_frequency
from .streams import input_desc, signal_desc


class TrackingLoop:
    def __init__(self, system: GNSSSystem, prns, num_samples: int, num_ants: int, sampling_frequency: float,
                 correlator_sample_shifts, init_carrier_doppler, init_code_phase, if_hz: float = 0.0,
                 carrier_center_hz: float = 1575.42e6, pll_bandwidth_hz: float = 18.0, dll_bandwidth_hz: float = 1.0,
                 init_carrier_phase=0.0, device=None, ctx: Context | None = None, weights=None):
        self.ctx = ctx if ctx is not None else get_context(device)
        self.ctx.set_codes(system.codes)
        self.system = system
        prns = np.atleast_1d(np.asarray(prns))
        self.K, self.N, self.M = int(prns.size), int(num_samples), int(num_ants)
        self.fs = float(sampling_frequency)
        self.shifts = np.ascontiguousarray(correlator_sample_shifts, dtype=np.int32)
        self.L = int(self.shifts.size)
        order = np.argsort(self.shifts, kind="stable")
        fc = get_code_frequency(system)
        cfg = _lib.LoopConfig()
        cfg.block_seconds = self.N / self.fs
        cfg.pll_bandwidth_hz, cfg.dll_bandwidth_hz = pll_bandwidth_hz, dll_bandwidth_hz
        cfg.code_freq_nominal_hz, cfg.carrier_center_hz, cfg.if_hz = fc, carrier_center_hz, if_hz
        cfg.code_length, cfg.num_taps = system.code_length, self.L
        cfg.early_index, cfg.late_index = int(order[0]), int(order[-1])
        zero = np.nonzero(self.shifts == 0)[0]
        if zero.size == 0:
            raise ValueError("the tap list needs a prompt tap (shift 0)")
        cfg.prompt_index = int(zero[0])
        cfg.early_late_spacing_chips = float(self.shifts[order[-1]] - self.shifts[order[0]]) * fc / self.fs
        self.config = cfg
        dop = np.broadcast_to(np.asarray(init_carrier_doppler, dtype=np.float64), (self.K,))
        prm = make_params(prns - 1, fc + dop * fc / carrier_center_hz, if_hz + dop, init_code_phase,
                          init_carrier_phase, shape=(1, self.K))
        dev = self.ctx.device
        self._params = [self.ctx.params_to_device(prm), self.ctx.params_to_device(prm)]
        self._cur = 0
        st = np.zeros(self.K, dtype=_lib.LOOP_STATE_DTYPE)
        st["init_carrier_doppler_hz"] = dop
        st["carrier_doppler_hz"] = dop
        self._state = torch.from_numpy(st.view(np.uint8).reshape(-1).copy()).to(dev)
        self.out_re = torch.empty((1, self.K, self.L, self.M), dtype=torch.float32, device=dev)
        self.out_im = torch.empty_like(self.out_re)
        self.blocks_done = 0
        self._w_re = self._w_im = None
        self.set_weights(weights)

    def set_weights(self, weights):
        """Beamformer weights complex [K, M] (``array.beamformer_weights``; a tensor or an array), or None: prompt, early and
        late become ``sum_m conj(w[k, m]) R[m, tap]`` instead of the plain sum over antennas.  The values are copied into
        buffers the loop keeps, so a graph recorded by ``run(graph=True)`` sees later weights too."""
        if weights is None:
            self._w_re = self._w_im = None
            return
        w = torch.as_tensor(weights).to(self.ctx.device)
        if tuple(w.shape) != (self.K, self.M):
            raise ValueError(f"weights must be [K, M] = [{self.K}, {self.M}]")
        w_re = (w.real if w.is_complex() else w).to(torch.float64)
        w_im = w.imag.to(torch.float64) if w.is_complex() else torch.zeros_like(w_re)
        if self._w_re is None:
            self._w_re, self._w_im = w_re.contiguous().clone(), w_im.contiguous().clone()
        else:
            self._w_re.copy_(w_re)
            self._w_im.copy_(w_im)

    def _weight_ptrs(self):
        if self._w_re is None:
            return None, None
        return C.c_void_p(self._w_re.data_ptr()), C.c_void_p(self._w_im.data_ptr())

    def step(self, re: torch.Tensor, im: torch.Tensor | None = None, start: int = 0):
        """Correlate the block starting at sample ``start`` of the given signal with the current
        parameters, then update them on the device.  Nothing is synchronised."""
        self.ctx.set_codes(self.system.codes)  # the context may have been bound to another system's table meanwhile
        desc = signal_desc(re, im, self.N, start=start)
        cur, nxt = self._params[self._cur], self._params[1 - self._cur]
        self.ctx.downconvert_and_correlate(desc, cur, 1, self.K, self.shifts, self.fs, self.out_re, self.out_im)
        args = (self.ctx._h, C.c_void_p(self.out_re.data_ptr()), C.c_void_p(self.out_im.data_ptr()), self.K, self.M,
                C.byref(self.config), C.c_void_p(self._state.data_ptr()), C.c_void_p(cur.data_ptr()), C.c_void_p(nxt.data_ptr()))
        if self._w_re is None:
            self.ctx.check(self.ctx.lib.gat_tracking_update(*args), "gat_tracking_update")
        else:
            self.ctx.check(self.ctx.lib.gat_tracking_update_weighted(*args, *self._weight_ptrs()), "gat_tracking_update_weighted")
        self._cur = 1 - self._cur
        self.blocks_done += 1

    def run(self, re: torch.Tensor, im: torch.Tensor | None, num_blocks: int, start: int = 0, keep: bool = True,
            graph: bool = False, out: tuple | None = None):
        """``num_blocks`` consecutive blocks (block b starts at sample start + b * N) through {correlate, update}
        in one native call (``gat_tracking_run``): the same launches as ``num_blocks`` x ``step`` without a
        host round trip per block.  Returns the accumulators of every block as device tensors (re, im)
        [num_blocks, K, L, M] when ``keep`` (into ``out`` = (re, im) if given), else only the last block's in
        ``out_re`` / ``out_im``.  ``graph``: GAT_FLAG_GRAPH -- calls that repeat with the same buffers replay an
        instantiated hipGraph (the context must be bound to a non-default stream)."""
        nb = int(num_blocks)
        self.ctx.set_codes(self.system.codes)  # the context may have been bound to another system's table meanwhile
        _, desc = input_desc((re, im), self.N, nb, start)
        if keep:
            if out is not None:
                acc_re, acc_im = out
            else:
                acc_re = torch.empty((nb, self.K, self.L, self.M), dtype=torch.float32, device=self.ctx.device)
                acc_im = torch.empty_like(acc_re)
            stride = self.K * self.L * self.M
        else:
            acc_re, acc_im, stride = self.out_re, self.out_im, 0
        a, b = self._params[self._cur], self._params[1 - self._cur]
        is_b = C.c_int32(0)
        args = (self.ctx._h, C.byref(desc), nb, self.K, self.L, self.shifts.ctypes.data_as(C.POINTER(C.c_int32)), self.fs,
                C.byref(self.config), C.c_void_p(self._state.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                C.c_void_p(acc_re.data_ptr()), C.c_void_p(acc_im.data_ptr()), stride, _lib.GAT_FLAG_GRAPH if graph else 0,
                C.byref(is_b))
        if self._w_re is None:
            self.ctx.check(self.ctx.lib.gat_tracking_run(*args), "gat_tracking_run")
        else:
            self.ctx.check(self.ctx.lib.gat_tracking_run_weighted(*args, *self._weight_ptrs()), "gat_tracking_run_weighted")
        if is_b.value:
            self._cur = 1 - self._cur
        self.blocks_done += nb
        if keep:
            self.out_re.copy_(acc_re[-1:])
            self.out_im.copy_(acc_im[-1:])
        return acc_re, acc_im

    def run_history(self, re: torch.Tensor, im: torch.Tensor | None, num_blocks: int, start: int = 0, out: tuple | None = None):
        """``run`` that keeps the parameters every block was correlated with (``gat_tracking_run_history``): returns ``(acc_re,
        acc_im, history)``, the accumulators of every block [num_blocks, K, L, M] (into ``out`` = (re, im) if given) and a uint8
        device tensor ``[num_blocks + 1, K, 40]`` of ``gat_channel_params`` records -- record 0 the parameters at entry, record b + 1
        what block b's update wrote.  The same launches and the same bits as ``run``; afterwards the loop's current parameters
        are record ``num_blocks``.  What ``observables`` reads."""
        nb = int(num_blocks)
        self.ctx.set_codes(self.system.codes)  # the context may have been bound to another system's table meanwhile
        _, desc = input_desc((re, im), self.N, nb, start)
        if out is not None:
            acc_re, acc_im = out
        else:
            acc_re = torch.empty((nb, self.K, self.L, self.M), dtype=torch.float32, device=self.ctx.device)
            acc_im = torch.empty_like(acc_re)
        cur = self._params[self._cur]
        history = torch.empty((nb + 1, self.K, 40), dtype=torch.uint8, device=self.ctx.device)
        history[0].view(-1).copy_(cur.view(torch.uint8).view(-1))
        rc = self.ctx.lib.gat_tracking_run_history(
            self.ctx._h, C.byref(desc), nb, self.K, self.L, self.shifts.ctypes.data_as(C.POINTER(C.c_int32)), self.fs, C.byref(self.config),
            C.c_void_p(self._state.data_ptr()), C.c_void_p(history.data_ptr()), C.c_void_p(acc_re.data_ptr()), C.c_void_p(acc_im.data_ptr()),
            self.K * self.L * self.M, 0, *self._weight_ptrs())
        self.ctx.check(rc, "gat_tracking_run_history")
        cur.view(torch.uint8).view(-1).copy_(history[nb].view(-1))
        self.blocks_done += nb
        self.out_re.copy_(acc_re[-1:])
        self.out_im.copy_(acc_im[-1:])
        return acc_re, acc_im, history

    def observables(self, history: torch.Tensor, mon, nav, **kw):
        """``observables.observables`` over a history of this loop (``run_history``), its monitor and its decoder's result, with the
        loop's block length, sampling rate, code, intermediate frequency and message format filled in; every keyword of that
        function may be given."""
        from .observables import observables

        kw.setdefault("ctx", self.ctx)
        return observables(history, mon, nav, loop=self, **kw)

    def monitor(self, acc_re: torch.Tensor, acc_im: torch.Tensor, **kw):
        """``monitor.monitor_accumulators`` over accumulators of this loop (``run(keep=True)``) with the loop's prompt tap, block
        length, beamformer weights and its system's overlay filled in; every keyword of that function may be given."""
        from .monitor import monitor_accumulators, overlay_for

        kw.setdefault("block_seconds", self.config.block_seconds)
        kw.setdefault("prompt_index", int(self.config.prompt_index))
        kw.setdefault("overlay", overlay_for(self.system))
        kw.setdefault("ctx", self.ctx)
        if self._w_re is not None:
            kw.setdefault("weights", (self._w_re, self._w_im))
        return monitor_accumulators(acc_re, acc_im, **kw)

    def navigation(self, mon, **kw):
        """``navigation.decode_navigation`` over a monitor of this loop (``monitor``) with the loop's system's message format
        filled in: frame synchronisation, polarity and the checked words; every keyword of that function may be given."""
        from .navigation import decode_navigation, nav_format_for

        kw.setdefault("format", nav_format_for(self.system))
        kw.setdefault("ctx", self.ctx)
        return decode_navigation(mon, **kw)

    def steering(self, acc_re: torch.Tensor, acc_im: torch.Tensor, **kw):
        """``subspace.steering_from_accumulators`` over accumulators of this loop (``run(keep=True)``) with the loop's prompt tap
        filled in: ``(steering [E, K, M], eigenvalues)`` on the device; every keyword of that function may be given."""
        from .subspace import steering_from_accumulators

        kw.setdefault("tap_index", int(self.config.prompt_index))
        kw.setdefault("ctx", self.ctx)
        return steering_from_accumulators(acc_re, acc_im, **kw)

    def params(self) -> np.ndarray:
        """Current per-channel parameters (host copy; synchronises)."""
        return self._params[self._cur].cpu().numpy().view(_lib.PARAMS_DTYPE).copy()

    def state(self) -> np.ndarray:
        return self._state.cpu().numpy().view(_lib.LOOP_STATE_DTYPE).copy()

    def accumulators(self) -> np.ndarray:
        """complex64 [K, L, M] of the last block."""
        return (self.out_re.cpu().numpy() + 1j * self.out_im.cpu().numpy())[0].astype(np.complex64)


class ResidentTrackingLoop:
    """The closed loop with the HOST in it, as in the reference's receiver (Tracking.jl's discriminators and loop filters run on
    the CPU): one step = one call rung into a resident correlator (``gat_resident_correlate``: no kernel launch, outputs
    arrive on the host) + ``gat_tracking_update_host`` (the arithmetic of the device's ``gat_tracking_update``, csrc/gat_loop.h)
    that turns the accumulators into the next block's parameters.  Same constructor as ``TrackingLoop`` plus the signal
    buffer the blocks live in; up to 16 channels.  ``run`` is the native loop (gat_resident_tracking_run)."""

    def __init__(self, system: GNSSSystem, prns, num_samples: int, num_ants: int, sampling_frequency: float,
                 correlator_sample_shifts, init_carrier_doppler, init_code_phase, re: torch.Tensor, im: torch.Tensor | None = None,
                 if_hz: float = 0.0, carrier_center_hz: float = 1575.42e6, pll_bandwidth_hz: float = 18.0,
                 dll_bandwidth_hz: float = 1.0, init_carrier_phase=0.0, device=None, ctx: Context | None = None, **resident_config):
        # the loop configuration, parameters and state: TrackingLoop's, kept on the host
        dev_loop = TrackingLoop(system, prns, num_samples, num_ants, sampling_frequency, correlator_sample_shifts, init_carrier_doppler,
                                init_code_phase, if_hz, carrier_center_hz, pll_bandwidth_hz, dll_bandwidth_hz, init_carrier_phase, device, ctx)
        self.ctx, self.system, self.config = dev_loop.ctx, system, dev_loop.config
        self.K, self.N, self.M, self.L, self.fs, self.shifts = dev_loop.K, dev_loop.N, dev_loop.M, dev_loop.L, dev_loop.fs, dev_loop.shifts
        self._cur = dev_loop.params().reshape(-1).copy()
        self._next = self._cur.copy()
        self._state = dev_loop.state().copy()
        self._signal = (re, im)  # kept alive: the resident kernel reads it
        desc = signal_desc(re, im, self.N, start=0)
        self._samples = int(re.shape[-2] if im is None else re.shape[-1])  # per antenna: every block has to end inside
        torch.cuda.current_stream(self.ctx.device).synchronize()  # the signal is on the device before the first ring
        self.resident = self.ctx.open_resident(desc, self.K, self.shifts, self.fs, buffer_samples=self._samples, **resident_config)
        self.resident_workgroups = self.resident.info()["workgroups"]
        self._lib = self.ctx.lib
        self._fn = self._lib.gat_tracking_update_host
        self.acc_re = self.acc_im = None
        self.blocks_done = 0

    def step(self, start: int = 0):
        """Correlate the block that starts ``start`` samples into the buffer with the current parameters, update them."""
        re, im = self.resident.correlate(self._cur, block_offset=start)
        rc = self._fn(C.c_void_p(re.ctypes.data), C.c_void_p(im.ctypes.data), self.K, self.M, C.byref(self.config),
                      C.c_void_p(self._state.ctypes.data), C.c_void_p(self._cur.ctypes.data), C.c_void_p(self._next.ctypes.data))
        host_check(rc, "gat_tracking_update_host")
        self._cur, self._next = self._next, self._cur
        self.acc_re, self.acc_im = re, im
        self.blocks_done += 1

    def run(self, num_blocks: int, start: int = 0, block_stride: int | None = None, keep_all: bool = False):
        """``num_blocks`` consecutive blocks from native code (``gat_resident_tracking_run``: {resident call, host update} per
        block without a trip through Python).  The blocks are ``block_stride`` samples apart (default: back to back) and all
        of them are on the device already.  ``keep_all``: returns complex64 [num_blocks, K, L, M] of every block's
        accumulators; otherwise only the last block's are kept (``accumulators()``)."""
        nb = int(num_blocks)
        if nb <= 0:
            return None
        n = self.K * self.L * self.M
        re = np.empty((nb if keep_all else 1, self.K, self.L, self.M), np.float32)
        im = np.empty_like(re)
        stride = self.N if block_stride is None else int(block_stride)
        # (the resident kernel reads the blocks with system-scope loads: a block outside the allocation is a GPU page fault)
        if start < 0 or stride < 0 or int(start) + (nb - 1) * stride + self.N > self._samples:
            raise ValueError("signal shorter than start + (num_blocks - 1) * block_stride + num_samples")
        rc = self._lib.gat_resident_tracking_run(self.resident._h, nb, int(start), stride, C.byref(self.config), C.c_void_p(self._state.ctypes.data),
                                                 C.c_void_p(self._cur.ctypes.data), C.c_void_p(re.ctypes.data), C.c_void_p(im.ctypes.data), n if keep_all else 0)
        self.ctx.check(rc, "gat_resident_tracking_run")
        self.acc_re, self.acc_im = re[-1], im[-1]
        self.blocks_done += nb
        return (re + 1j * im).astype(np.complex64) if keep_all else None

    def params(self) -> np.ndarray:
        return self._cur.copy()

    def state(self) -> np.ndarray:
        return self._state.copy()

    def accumulators(self) -> np.ndarray:
        """complex64 [K, L, M] of the last block."""
        return (self.acc_re + 1j * self.acc_im).astype(np.complex64)

    def close(self):
        self.resident.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
