"""Signal acquisition: the GPU search over PRN x Doppler x code phase that finds which satellites are present and where,
and seeds the tracking loops (``TrackingLoop``, ``ResidentTrackingLoop``) with it.  Modelled on Acquisition.jl's
``acquire(system, signal, sampling_frequency, prns; interm_freq, max_doppler, dopplers)`` and its ``AcquisitionResults``.

The search runs in libgat (``gat_acquire``, csrc/gat_acq.hip): for every PRN, Doppler bin f_i and code bin j,

    P[p, i, j] = sum over blocks and antennas of |R|^2,

R being what the correlator returns for the channel {p, fc, interm_freq + f_i, tau_b, 0} and the tap first_shift + s j
(include/gat.h states the contract).  A coarse search covers one code period in half-chip bins and +-max_doppler; an
explicit ``first_shift`` / ``num_code_bins`` and a narrow ``dopplers`` range around a coarse estimate make the same call a
fine search (with a block of several code periods, bins of 10-50 Hz)."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field

import numpy as np
import torch

from . import _lib
from .array import beamform_desc
from .context import Context, get_context
from .gen_signal import make_params
from .results import host_check, new_plan, plan_report
from .signals import GNSSSystem, get_code_frequency
from .streams import input_desc, ref, vp


@dataclass
class AcquisitionResult:
    """One PRN's search result (Acquisition.jl's AcquisitionResults: prn, sampling_frequency, carrier_doppler, code_phase,
    CN0, noise_power, signal_power, power_bins, dopplers).  ``prn`` is the 0-based code-table column searched (the
    reference's PRN minus one); ``detected`` is 1 / 0, or -1 when the grid was too narrow for a noise estimate."""

    prn: int
    sampling_frequency: float
    carrier_doppler: float
    code_phase: float
    CN0: float
    noise_power: float
    signal_power: float
    peak_to_second: float
    second_power: float
    detected: int
    doppler_bin: int
    code_bin: int
    power_bins: torch.Tensor | None = field(default=None, repr=False)  # [D, J] on the device (keep_power=True)
    dopplers: np.ndarray | None = field(default=None, repr=False)


def _as_desc(signal, num_samples: int, num_blocks: int, block_stride: int):
    """``signal``: planar (re, im) float32 tensors [M, Ntot], or one interleaved tensor [M, Ntot, 2] of float32, int16 or
    int8 pairs, on the device; or a ready gat_signal_desc (then ``num_samples`` etc. are taken from it)."""
    return signal if isinstance(signal, _lib.SignalDesc) else input_desc(signal, num_samples, num_blocks, 0, block_stride)[1]


def acquire(system: GNSSSystem, signal, sampling_frequency: float, prns=range(32), *, num_samples: int | None = None,
            interm_freq: float = 0.0, max_doppler: float = 7000.0, doppler_step: float | None = None, dopplers=None,
            code_step_chips: float | None = 0.5, first_shift: int = 0, num_code_bins: int | None = None, num_blocks: int = 1,
            block_stride: int | None = None, min_peak_ratio: float = 2.0, keep_power: bool = False,
            ctx: Context | None = None, device=None, weights=None, method: str = "direct") -> list[AcquisitionResult]:
    """Search ``prns`` (code-table columns, 0-based) in ``num_blocks`` blocks of ``num_samples`` samples (default: one
    code period) starting at sample 0 of ``signal``, ``block_stride`` apart (default ``num_samples``).

    Grid defaults: code step s = max(1, round(code_step_chips * fs / fc)) samples, J = ceil(Lc * fs / (fc * s)) bins (one
    code period) from ``first_shift``; Doppler -max_doppler .. +max_doppler in steps of 1 / (2 N / fs), or the evenly
    spaced ``dopplers`` given (Hz, relative to ``interm_freq``).  Returns one AcquisitionResult per PRN, in order.

    ``weights`` (complex ``[J, M]`` or ``[M]``, e.g. ``beamformer_weights(R, mode="power_inversion")``): the blocks searched
    are first beamformed (``array.beamform_samples``'s ``beamform_desc``, into a buffer that lives for this call) and the search runs on the J
    beams, non-coherently over them as it is over antennas.  The search adds antennas as |R|^2, so a jammer that is coherent
    across them enters at full strength; a beam with a null towards it does not.  With power-inversion weights the result's
    ``CN0``, ``noise_power`` and ``signal_power`` are those of the beam's output (its noise is sum |w_m|^2 times one
    antenna's, and the satellite's gain is whatever the null leaves), not of an antenna.  ``weights=None``: the search on
    the antennas as they are.

    ``method``: ``"direct"`` (``gat_acquire``: one sum per bin; the default) or ``"fft"`` (``gat_acquire_fft``: every lag of a block
    from transforms of F > N points -- the same grid under the same contract, within the same 1e-5 of it, not bit-equal to the
    direct search).  The FFT search costs the same whatever the code step, so with ``method="fft"`` and ``code_step_chips=None``
    the grid is sample-spaced: s = 1 and J = one code period of samples.  Choose it for s = 1, for long codes (GPS L5) and for many
    non-coherent blocks; the direct search wins on coarse grids (DESIGN.md 4.6 has the measured ratios).  Blocks of 2^18 samples
    and more are refused."""
    if method not in ("direct", "fft"):
        raise ValueError("method must be 'direct' or 'fft'")
    if code_step_chips is None:
        if method != "fft":
            raise ValueError("code_step_chips=None (sample spacing) needs method='fft'")
    ctx = ctx if ctx is not None else get_context(device)
    ctx.set_codes(system.codes)
    fs = float(sampling_frequency)
    fc = get_code_frequency(system)
    lc = int(system.code_length)
    N = int(num_samples) if num_samples is not None else int(math.ceil(lc * fs / fc))
    bstride = int(block_stride) if block_stride is not None else N
    if isinstance(signal, _lib.SignalDesc):
        N = int(signal.num_samples)
    s = 1 if code_step_chips is None else max(1, int(round(code_step_chips * fs / fc)))
    J = int(num_code_bins) if num_code_bins is not None else int(math.ceil(lc * fs / (fc * s)))
    if dopplers is None:
        step = float(doppler_step) if doppler_step is not None else fs / (2.0 * N)
        nd = int(math.floor(max_doppler / step + 1e-9))
        dop = np.arange(-nd, nd + 1, dtype=np.float64) * step
    else:
        dop = np.asarray(dopplers, dtype=np.float64).reshape(-1)
        if dop.size > 1 and not np.allclose(np.diff(dop), dop[1] - dop[0], rtol=1e-9, atol=1e-9):
            raise ValueError("dopplers must be evenly spaced")
    D = int(dop.size)
    fstep = float(dop[1] - dop[0]) if D > 1 else 0.0
    prn_arr = np.ascontiguousarray(np.asarray(list(prns) if not isinstance(prns, np.ndarray) else prns, dtype=np.int32).reshape(-1))
    P = int(prn_arr.size)
    desc = _as_desc(signal, N, int(num_blocks), bstride)
    if weights is not None:
        if desc.chan_stride != 0:
            raise ValueError("weights need one signal for all channels (chan_stride 0)")
        beams, desc = beamform_desc(ctx, desc, weights, int(num_blocks), zero=False)  # `beams` lives until gat_acquire has returned

    cfg = _lib.AcqConfig()
    cfg.struct_size = C.sizeof(_lib.AcqConfig)
    cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples = D, J, s
    cfg.if_hz, cfg.code_freq_hz = float(interm_freq), fc
    cfg.doppler_first_hz, cfg.doppler_step_hz = float(dop[0]) if D else 0.0, fstep
    cfg.first_shift, cfg.min_peak_ratio, cfg.code_length = int(first_shift), float(min_peak_ratio), lc

    power = torch.empty((P, D, J), dtype=torch.float32, device=ctx.device) if keep_power else None
    res = np.zeros(max(P, 1), dtype=_lib.ACQ_RESULT_DTYPE)
    name = "gat_acquire_fft" if method == "fft" else "gat_acquire"
    rc = getattr(ctx.lib, name)(ctx._h, C.byref(desc), int(num_blocks), prn_arr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs,
                                C.byref(cfg), vp(power), C.c_void_p(res.ctypes.data))
    ctx.check(rc, name)
    out = []
    for p in range(P):
        r = res[p]
        out.append(AcquisitionResult(
            prn=int(r["prn"]), sampling_frequency=fs, carrier_doppler=float(r["carrier_doppler_hz"]),
            code_phase=float(r["code_phase_chips"]), CN0=float(r["cn0_dbhz"]), noise_power=float(r["noise_power"]),
            signal_power=float(r["peak_power"]), peak_to_second=float(r["peak_to_second"]),
            second_power=float(r["second_power"]), detected=int(r["detected"]), doppler_bin=int(r["doppler_bin"]),
            code_bin=int(r["code_bin"]), power_bins=power[p] if power is not None else None, dopplers=dop))
    return out


def acquire_fft_plan(desc: _lib.SignalDesc, num_blocks: int, num_prns: int, sampling_frequency: float, config: _lib.AcqConfig, *,
                     fft_log2: int = 0, doppler_batch: int = 0, unit_batch: int = 0, num_cus: int = 256, own_power: bool = False) -> dict:
    """``gat_acquire_fft_plan``: what ``gat_acquire_fft`` would do with this call (transform length, lag segments, passes, batches,
    unit groups, scratch bytes), without a device.  ``num_cus``: the device's compute units (``Context.device_info()``); the three
    options as ``Context.set_option`` would set them.  Raises ``GatError`` with the refusal the call would get."""
    plan = new_plan(_lib.AcqFftPlan)
    rc = _lib.load().gat_acquire_fft_plan(ref(desc), int(num_blocks), int(num_prns), float(sampling_frequency), ref(config), int(fft_log2),
                                          int(doppler_batch), int(unit_batch), int(num_cus), int(bool(own_power)), C.byref(plan))
    host_check(rc, "gat_acquire_fft_plan")
    return plan_report(plan)


def acquire_fft_host(desc: _lib.SignalDesc, num_blocks: int, codes: np.ndarray, prns, sampling_frequency: float, config: _lib.AcqConfig,
                     fft_log2: int, unit_groups: int = 1) -> np.ndarray:
    """``gat_acquire_fft_host``: the FFT search's grid [P, D, J] on the host over a descriptor of HOST memory (``streams.host_desc``),
    bit for bit the device's for the same ``fft_log2`` and ``unit_groups``.  ``codes``: int8 [rows, Lc]; ``prns``: rows."""
    tab = np.ascontiguousarray(codes, dtype=np.int8)
    if tab.ndim != 2:
        raise ValueError("codes must be [rows, code_length]")
    prn_arr = np.ascontiguousarray(np.asarray(prns, dtype=np.int32).reshape(-1))
    P = int(prn_arr.size)
    power = np.zeros((max(P, 1), max(int(config.num_doppler_bins), 1), max(int(config.num_code_bins), 1)), dtype=np.float32)
    rc = _lib.load().gat_acquire_fft_host(C.byref(desc), int(num_blocks), C.c_void_p(tab.ctypes.data), int(tab.shape[1]), int(tab.shape[1]),
                                          prn_arr.ctypes.data_as(C.POINTER(C.c_int32)), P, float(sampling_frequency), C.byref(config),
                                          int(fft_log2), int(unit_groups), C.c_void_p(power.ctypes.data))
    host_check(rc, "gat_acquire_fft_host")
    return power


def acquisition_stats_host(power: np.ndarray, config: _lib.AcqConfig, sampling_frequency: float,
                           num_samples: int) -> np.ndarray:
    """``gat_acq_stats_host``: the search's per-PRN statistics over a host grid [P, D, J] (structured array of
    gat_acq_result; ``prn`` is the row index)."""
    g = np.ascontiguousarray(power, dtype=np.float32)
    if g.ndim != 3:
        raise ValueError("power must be [num_prns, num_doppler_bins, num_code_bins]")
    P, D, J = g.shape
    res = np.zeros(max(P, 1), dtype=_lib.ACQ_RESULT_DTYPE)
    rc = _lib.load().gat_acq_stats_host(C.c_void_p(g.ctypes.data), P, D, J, C.byref(config), float(sampling_frequency),
                                        int(num_samples), C.c_void_p(res.ctypes.data))
    host_check(rc, "gat_acq_stats_host")
    return res[:P]


def tracking_init(results, system: GNSSSystem, if_hz: float = 0.0, carrier_center_hz: float = 1575.42e6,
                  detected_only: bool = True) -> dict:
    """The detected results as tracking-loop initial values: ``prns`` (1-based, as ``TrackingLoop`` takes them),
    ``init_carrier_doppler``, ``init_code_phase`` and ``params`` -- ``make_params`` records (carrier phase 0; the code
    frequency carrier-aided as the loop does) for the correlator."""
    sel = [r for r in results if (r.detected == 1 or not detected_only)]
    fc = get_code_frequency(system)
    prn0 = np.array([r.prn for r in sel], dtype=np.int32)
    dop = np.array([r.carrier_doppler for r in sel], dtype=np.float64)
    tau = np.array([r.code_phase for r in sel], dtype=np.float64)
    params = make_params(prn0, fc + dop * fc / carrier_center_hz, if_hz + dop, tau, 0.0, shape=(1, prn0.size))
    return dict(prns=prn0 + 1, init_carrier_doppler=dop, init_code_phase=tau, params=params)
