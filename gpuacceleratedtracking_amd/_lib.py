"""ctypes binding of libgat.so -- the only way the Python host layer reaches the GPU.

There is NO fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

GAT_OK = 0
GAT_FLAG_ATOMIC = 1
GAT_FLAG_GRAPH = 2
GAT_LAYOUT_PLANAR = 0
GAT_LAYOUT_INTERLEAVED = 1
GAT_LAYOUT_INTERLEAVED_I16 = 2
GAT_LAYOUT_INTERLEAVED_I8 = 3
# bytes of one complex sample per layout
SAMPLE_BYTES = {0: 8, 1: 8, 2: 4, 3: 2}
GAT_MAX_TAPS = 32
# kernel selection (gat_set_matrix_core)
GAT_MC_VECTOR, GAT_MC_AUTO, GAT_MC_F32, GAT_MC_BF16_SPLIT = 0, 1, 2, 3
# antenna-array processing (gat_array_weights modes; the array functions' antenna limit)
GAT_BF_CONVENTIONAL, GAT_BF_MVDR, GAT_BF_POWER_INVERSION = 0, 1, 2
GAT_MAX_ARRAY_ANTS = 64
# sample conditioning (gat_condition_samples / gat_sample_stats flags)
GAT_COND_BLANK_ALL_ANTS = 1
# sample filtering (gat_filter_samples limits)
GAT_MAX_FIR_TAPS, GAT_MAX_FIR_DECIMATION = 256, 64
# sample spectrum (gat_sample_spectrum limits)
GAT_MIN_SPECTRUM_BINS, GAT_MAX_SPECTRUM_BINS, GAT_MAX_SPECTRUM_SEGMENTS = 64, 4096, 4096
# space-time adaptive processing (taps per antenna; num_ants * num_taps <= GAT_MAX_ARRAY_ANTS)
GAT_MAX_ST_TAPS = 16
# tracking monitor (gat_track_monitor limits)
GAT_MAX_SYMBOL_BLOCKS, GAT_MAX_MONITOR_BLOCKS, GAT_MAX_MONITOR_CHANNELS = 128, 1 << 20, 4096
# subspace (gat_accumulator_covariance's chunk, gat_hermitian_eig's sweep limit and input flag)
GAT_ACC_COV_CHUNK, GAT_EIG_MAX_SWEEPS, GAT_EIG_INPUT_F32 = 256, 60, 1
# navigation data (gat_nav_decode formats, the frame length and CNAV's unsearched traceback tail)
GAT_NAV_LNAV, GAT_NAV_CNAV, GAT_NAV_FRAME_BITS, GAT_NAV_TAIL_BITS = 0, 1, 300, 32
# position fix (gat_position_fix limits, the status bits of gat_fix and the reasons of gat_lnav_ephemeris_host)
GAT_MAX_FIX_CHANNELS, GAT_MAX_FIX_EPOCHS = 64, 1 << 24
GAT_FIX_FEW_SATS, GAT_FIX_SINGULAR, GAT_FIX_NONFINITE, GAT_FIX_NOT_CONVERGED, GAT_FIX_MASK_STARVED, GAT_FIX_MASKED = 1, 2, 4, 8, 16, 32
GAT_EPH_OK, GAT_EPH_MISSING, GAT_EPH_IODE = 0, 1, 2
# observables (the status bits of gat_obs_channel and the reception modes of gat_obs_config)
GAT_OBS_BAD_RECORD, GAT_OBS_NO_BIT_SYNC, GAT_OBS_NO_FRAME_SYNC, GAT_OBS_FRAME_OUTSIDE, GAT_OBS_NO_TOW, GAT_OBS_EDGE_AMBIGUOUS = 1, 2, 4, 8, 16, 32
GAT_OBS_RX_GIVEN, GAT_OBS_RX_FROM_TX = 0, 1
# fix integrity (the status bits of gat_fix_integrity, the bit gat_position_fix_raim adds to gat_fix.status, the rounds' limit)
GAT_RAIM_NOT_CHECKED, GAT_RAIM_NO_REDUNDANCY, GAT_RAIM_DETECTED, GAT_RAIM_EXCLUDED, GAT_RAIM_UNRESOLVED = 1, 2, 4, 8, 16
GAT_FIX_EXCLUDED, GAT_RAIM_MAX_EXCLUDE = 64, 4
# velocity fix (the status bits of gat_velocity)
GAT_VEL_FEW_SATS, GAT_VEL_SINGULAR, GAT_VEL_NONFINITE, GAT_VEL_NO_FIX, GAT_VEL_NO_GEODETIC = 1, 2, 4, 8, 16
# atmosphere (the flags of gat_atm_config, the bits of epoch_status and of channel_status)
GAT_ATM_IONO, GAT_ATM_TROPO = 1, 2
GAT_ATM_NO_FIX, GAT_ATM_NO_GEODETIC = 1, 2
GAT_ATM_CH_CORRECTED, GAT_ATM_CH_LOW, GAT_ATM_CH_NONFINITE = 1, 2, 4
# carrier smoothing (the flag of gat_smooth_config, the bits of status, the limit on the epochs)
GAT_SMOOTH_RATE_TEST = 1
GAT_SMOOTH_MEASURED, GAT_SMOOTH_GAP, GAT_SMOOTH_CMC, GAT_SMOOTH_RATE = 1, 2, 4, 8
GAT_MAX_SMOOTH_EPOCHS = 1048576
# snapshot fix (the status bits of gat_snap_fix)
(GAT_SNAP_FEW_SATS, GAT_SNAP_SINGULAR, GAT_SNAP_NONFINITE, GAT_SNAP_NOT_CONVERGED, GAT_SNAP_MASK_STARVED, GAT_SNAP_MASKED, GAT_SNAP_AMBIGUOUS,
 GAT_SNAP_RERESOLVED) = 1, 2, 4, 8, 16, 32, 64, 128

EXPORTS = [
    "gat_create", "gat_destroy", "gat_set_stream", "gat_sync", "gat_last_error", "gat_version",
    "gat_device_info", "gat_set_codes", "gat_gen_codes", "gat_sample_shifts",
    "gat_downconvert_and_correlate", "gat_downconvert_and_correlate_dev", "gat_gen_code_replica",
    "gat_gen_code_replica_f32coord",
    "gat_gen_signal", "gat_reduce_cplx_multi", "gat_tracking_update", "gat_malloc", "gat_free", "gat_memcpy_h2d",
    "gat_memcpy_d2h", "gat_memset", "gat_timer_start", "gat_timer_stop", "gat_last_launch_info", "gat_set_matrix_core", "gat_tracking_run", "gat_set_vector_tiling", "gat_gen_code_replica_multi",
    "gat_downconvert_and_accumulate", "gat_gen_signal_noisy", "gat_set_option",
    # several devices from one host thread (channel sharding, no collective)
    "gat_device_count", "gat_memcpy_peer", "gat_group_create", "gat_group_destroy", "gat_group_size", "gat_group_ctx",
    "gat_group_last_error", "gat_group_shard", "gat_group_set_codes", "gat_group_replicate", "gat_group_correlate",
    "gat_group_gather", "gat_group_sync",
    # resident correlator: single-block calls without a kernel launch
    "gat_resident_open", "gat_resident_correlate", "gat_resident_info_get", "gat_resident_park", "gat_resident_close",
    "gat_tracking_update_host", "gat_resident_tracking_run", "gat_resident_park_all",
    # measurement: per-call statistics, the in-run read ceiling; the texture-addressing study
    "gat_timer_lap", "gat_timer_laps", "gat_debug_read_stream", "gat_gen_code_replica_texaddr",
    # acquisition: the PRN x Doppler x code-phase search that seeds the tracking loops
    "gat_acquire", "gat_acq_stats_host", "gat_acquire_fft", "gat_acquire_fft_plan", "gat_acquire_fft_host",
    # antenna-array processing: spatial covariance, beamformer weights, beamformed accumulators and loop
    "gat_spatial_covariance", "gat_array_weights", "gat_array_weights_host", "gat_beamform", "gat_tracking_update_weighted",
    "gat_tracking_update_host_weighted", "gat_tracking_run_weighted", "gat_beamform_samples",
    # sample conditioning: level statistics, pulse blanking, AGC, requantisation
    "gat_condition_samples", "gat_condition_samples_host", "gat_sample_stats", "gat_agc_update", "gat_agc_update_host",
    # sample filtering: complex FIR, decimation and an oscillator over the raw samples
    "gat_filter_samples", "gat_filter_samples_host",
    # sample spectrum: the summed periodogram of the raw samples per block and antenna
    "gat_sample_spectrum", "gat_sample_spectrum_host",
    # space-time adaptive processing: the tapped covariance and the space-time sample filter
    "gat_spacetime_covariance", "gat_spacetime_filter", "gat_spacetime_filter_host",
    # tracking monitor: C/N0, phase lock, bit synchronisation and data symbols from the accumulator history
    "gat_track_monitor", "gat_track_monitor_host", "gat_track_monitor_plan",
    # subspace: the accumulators' covariance, the batched Hermitian eigensolver and their plan
    "gat_accumulator_covariance", "gat_accumulator_covariance_host", "gat_hermitian_eig", "gat_hermitian_eig_host",
    "gat_subspace_plan",
    # navigation data: frame synchronisation, LNAV parity, CNAV Viterbi decoding and CRC-24Q
    "gat_nav_decode", "gat_nav_decode_host", "gat_nav_decode_plan",
    # position fix: LNAV ephemeris, satellite states and the batched least-squares solver
    "gat_position_fix", "gat_position_fix_host", "gat_position_fix_plan", "gat_lnav_ephemeris_host", "gat_lnav_ephemeris_words_host",
    # observables: the loop's parameter history, transmit times and carrier phase from it
    "gat_tracking_run_history", "gat_observables", "gat_observables_host", "gat_observables_plan",
    # fix integrity: the residual test and fault exclusion on top of the position fix
    "gat_position_fix_raim", "gat_position_fix_raim_host", "gat_position_fix_raim_plan",
    # velocity fix: satellite velocities, the Doppler solver and the local frame
    "gat_velocity_fix", "gat_velocity_fix_host", "gat_velocity_fix_plan",
    # atmosphere: Klobuchar and troposphere delays, corrected transmit times, subframe 4 page 18
    "gat_range_corrections", "gat_range_corrections_host", "gat_range_corrections_plan", "gat_atm_atan2_host",
    "gat_lnav_page18_host", "gat_lnav_page18_words_host",
    # carrier smoothing: cycle-slip arcs and Hatch-filtered transmit times
    "gat_smooth_observables", "gat_smooth_observables_host", "gat_smooth_observables_plan",
    # snapshot fix: a coarse-time position from code phases alone
    "gat_snapshot_fix", "gat_snapshot_fix_host", "gat_snapshot_fix_plan",
]


class GatError(RuntimeError):
    """A libgat call returned a non-zero status."""

    def __init__(self, status: int, where: str, message: str = ""):
        self.status = status
        kind = {1: "GAT_ERR_ARG", 2: "GAT_ERR_RANGE", 3: "GAT_ERR_STATE", 4: "GAT_ERR_UNSUPPORTED",
                5: "GAT_ERR_NOMEM"}.get(status, f"hipError {-status}" if status < 0 else str(status))
        super().__init__(f"{where}: {kind}" + (f" ({message})" if message else ""))


class ChannelParams(C.Structure):
    """gat_channel_params (include/gat.h)."""

    _fields_ = [("prn", C.c_int32), ("reserved", C.c_int32), ("code_freq_hz", C.c_double),
                ("carrier_freq_hz", C.c_double), ("code_phase_chips", C.c_double),
                ("carrier_phase_cycles", C.c_double)]


PARAMS_DTYPE = np.dtype([("prn", "<i4"), ("reserved", "<i4"), ("code_freq_hz", "<f8"),
                         ("carrier_freq_hz", "<f8"), ("code_phase_chips", "<f8"),
                         ("carrier_phase_cycles", "<f8")])
assert PARAMS_DTYPE.itemsize == C.sizeof(ChannelParams) == 40


class SignalDesc(C.Structure):
    """gat_signal_desc (include/gat.h)."""

    _fields_ = [("re", C.c_void_p), ("im", C.c_void_p), ("layout", C.c_int32),
                ("num_ants", C.c_int32), ("num_samples", C.c_int64), ("ant_stride", C.c_int64),
                ("block_stride", C.c_int64), ("chan_stride", C.c_int64)]


class LoopConfig(C.Structure):
    """gat_loop_config (include/gat.h)."""

    _fields_ = [("block_seconds", C.c_double), ("pll_bandwidth_hz", C.c_double), ("dll_bandwidth_hz", C.c_double),
                ("code_freq_nominal_hz", C.c_double), ("carrier_center_hz", C.c_double), ("if_hz", C.c_double),
                ("early_late_spacing_chips", C.c_double), ("code_length", C.c_int32), ("num_taps", C.c_int32),
                ("early_index", C.c_int32), ("prompt_index", C.c_int32), ("late_index", C.c_int32)]


LOOP_STATE_DTYPE = np.dtype([(n, "<f8") for n in (
    "init_carrier_doppler_hz", "carrier_doppler_hz", "code_doppler_hz", "pll_acc1", "pll_acc2", "dll_acc",
    "last_pll_error_cycles", "last_dll_error_chips", "prompt_power")])


class LaunchInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("workgroups", "threads", "splits", "ant_tile", "vec",
                                          "lds_bytes", "finalize_launched", "matrix_core", "channels_per_wg",
                                          "blocks_per_wg", "prefetch_depth", "bf16_terms")]


class ResidentConfig(C.Structure):
    """gat_resident_config (include/gat.h)."""

    _fields_ = [(n, C.c_uint32) for n in ("struct_size", "idle_us", "life_ms", "max_calls", "max_workgroups", "host_pollers", "doorbell")]


class ResidentInfo(C.Structure):
    """gat_resident_info (include/gat.h)."""

    _fields_ = [("workgroups", C.c_int32), ("splits", C.c_int32), ("running", C.c_int32), ("last_exit", C.c_int32),
                ("launches", C.c_uint64), ("calls", C.c_uint64)]


class AcqConfig(C.Structure):
    """gat_acq_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_doppler_bins", C.c_int32), ("if_hz", C.c_double),
                ("code_freq_hz", C.c_double), ("doppler_first_hz", C.c_double), ("doppler_step_hz", C.c_double),
                ("first_shift", C.c_int64), ("code_step_samples", C.c_int32), ("num_code_bins", C.c_int32),
                ("min_peak_ratio", C.c_double), ("code_length", C.c_int32), ("reserved", C.c_int32)]


ACQ_RESULT_DTYPE = np.dtype([("prn", "<i4"), ("detected", "<i4"), ("doppler_bin", "<i4"), ("code_bin", "<i4"),
                             ("peak_power", "<f8"), ("noise_power", "<f8"), ("second_power", "<f8"),
                             ("peak_to_second", "<f8"), ("cn0_dbhz", "<f8"), ("carrier_doppler_hz", "<f8"),
                             ("code_phase_chips", "<f8"), ("num_noise_bins", "<i8")])
assert C.sizeof(AcqConfig) == 72 and ACQ_RESULT_DTYPE.itemsize == 80


class AcqFftPlan(C.Structure):
    """gat_acq_fft_plan (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("fft_log2", C.c_int32), ("num_segments", C.c_int32), ("segment_lags", C.c_int32),
                ("passes", C.c_int32), ("doppler_batch", C.c_int32), ("unit_batch", C.c_int32), ("unit_groups", C.c_int32),
                ("scratch_bytes", C.c_int64)]


assert C.sizeof(AcqFftPlan) == 40


class AgcConfig(C.Structure):
    """gat_agc_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("target_rms", C.c_double), ("blank_factor", C.c_double), ("remove_dc", C.c_int32)]


# gat_cond_params and gat_sample_stats_t (include/gat.h)
COND_PARAMS_DTYPE = np.dtype([("scale", "<f4"), ("dc_re", "<f4"), ("dc_im", "<f4"), ("threshold", "<f4")])
SAMPLE_STATS_DTYPE = np.dtype([("kept", "<i8"), ("blanked", "<i8"), ("sum_re", "<f8"), ("sum_im", "<f8"), ("sum_pow", "<f8"),
                               ("max_abs", "<f4"), ("pad_", "<f4")])
assert C.sizeof(AgcConfig) == 32 and COND_PARAMS_DTYPE.itemsize == 16 and SAMPLE_STATS_DTYPE.itemsize == 48


class FirConfig(C.Structure):
    """gat_fir_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_taps", C.c_int32), ("decimation", C.c_int32), ("nco_step", C.c_double),
                ("nco_phase", C.c_double)]


assert C.sizeof(FirConfig) == 32


class SpectrumConfig(C.Structure):
    """gat_spectrum_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_bins", C.c_int32), ("hop", C.c_int32), ("flags", C.c_uint32)]


assert C.sizeof(SpectrumConfig) == 16


class MonitorConfig(C.Structure):
    """gat_monitor_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_taps", C.c_int32), ("prompt_index", C.c_int32), ("window_blocks", C.c_int32),
                ("symbol_blocks", C.c_int32), ("symbol_offset", C.c_int32), ("first_block", C.c_int64), ("overlay", C.c_int8 * 128)]


class MonitorPlan(C.Structure):
    """gat_monitor_plan (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_windows", C.c_int32), ("search_symbols", C.c_int32), ("symbol_capacity", C.c_int32),
                ("prompt_workgroups", C.c_int32), ("window_workgroups", C.c_int32), ("term_workgroups", C.c_int32),
                ("energy_workgroups", C.c_int32), ("pick_workgroups", C.c_int32), ("symbol_workgroups", C.c_int32),
                ("scratch_bytes", C.c_int64)]


class SubspacePlan(C.Structure):
    """gat_subspace_plan_info (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_estimates", C.c_int32), ("chunks_per_estimate", C.c_int32), ("cov_split", C.c_int32),
                ("cov_workgroups", C.c_int32), ("cov_threads", C.c_int32), ("cov_lds_bytes", C.c_int32), ("cov_reduce_workgroups", C.c_int32),
                ("eig_workgroups", C.c_int32), ("eig_threads", C.c_int32), ("eig_lds_bytes", C.c_int32), ("reserved", C.c_int32),
                ("scratch_bytes", C.c_int64)]


assert C.sizeof(SubspacePlan) == 56

# gat_monitor_window and gat_monitor_channel (include/gat.h)
MONITOR_WINDOW_DTYPE = np.dtype([("sum_p2", "<f8"), ("sum_p4", "<f8"), ("sum_d", "<f8"), ("sum_i", "<f8"), ("sum_q", "<f8"), ("blocks", "<i8")])
MONITOR_CHANNEL_DTYPE = np.dtype([("symbol_offset", "<i4"), ("start", "<i4"), ("num_symbols", "<i4"), ("reserved", "<i4"),
                                  ("e_max", "<f8"), ("e_second", "<f8")])
assert C.sizeof(MonitorConfig) == 160 and C.sizeof(MonitorPlan) == 48
assert MONITOR_WINDOW_DTYPE.itemsize == 48 and MONITOR_CHANNEL_DTYPE.itemsize == 32


class NavConfig(C.Structure):
    """gat_nav_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_int32), ("symbol_capacity", C.c_int32), ("max_frames", C.c_int32),
                ("min_frames", C.c_int32)]


class NavPlan(C.Structure):
    """gat_nav_plan (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("num_phases", C.c_int32), ("bit_capacity", C.c_int32), ("num_candidates", C.c_int32),
                ("slice_workgroups", C.c_int32), ("quantise_workgroups", C.c_int32), ("trellis_workgroups", C.c_int32),
                ("score_workgroups", C.c_int32), ("pick_workgroups", C.c_int32), ("frame_workgroups", C.c_int32),
                ("scratch_bytes", C.c_int64)]


# gat_nav_channel and gat_nav_frame (include/gat.h)
NAV_CHANNEL_DTYPE = np.dtype([(n, "<i4") for n in ("frame_offset", "symbol_phase", "inverted", "score", "second_score", "num_frames",
                                                    "num_bits", "tow_steps")])
NAV_FRAME_DTYPE = np.dtype([("status", "<i4"), ("tow", "<i4"), ("id", "<i4"), ("prn", "<i4"), ("words", "<u4", (10,))])
assert C.sizeof(NavConfig) == 20 and C.sizeof(NavPlan) == 48 and NAV_CHANNEL_DTYPE.itemsize == 32 and NAV_FRAME_DTYPE.itemsize == 56


class FixConfig(C.Structure):
    """gat_fix_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("max_iter", C.c_int32), ("tol_m", C.c_double), ("mask_sin", C.c_double),
                ("init_xyz", C.c_double * 3), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class FixPlan(C.Structure):
    """gat_fix_plan (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("workgroups", C.c_int32), ("waves_per_workgroup", C.c_int32), ("threads", C.c_int32),
                ("lds_bytes", C.c_int32), ("reserved", C.c_int32), ("scratch_bytes", C.c_int64)]


# gat_ephemeris and gat_fix (include/gat.h)
EPHEMERIS_INTS = ("wn", "iodc", "iode", "health", "ura", "fit")
EPHEMERIS_DOUBLES = ("toc", "toe", "af0", "af1", "af2", "tgd", "sqrt_a", "e", "m0", "delta_n", "omega0", "i0", "omega", "omega_dot", "idot",
                     "cuc", "cus", "crc", "crs", "cic", "cis")
EPHEMERIS_DTYPE = np.dtype([(n, "<i4") for n in EPHEMERIS_INTS] + [(n, "<f8") for n in EPHEMERIS_DOUBLES] + [("valid", "<i4"), ("reason", "<i4")])
FIX_DTYPE = np.dtype([("status", "<i4"), ("num_valid", "<i4"), ("num_used", "<i4"), ("iterations", "<i4"), ("x", "<f8"), ("y", "<f8"),
                      ("z", "<f8"), ("clock_bias_s", "<f8"), ("rms_residual_m", "<f8"), ("last_step_m", "<f8"), ("gdop", "<f8"), ("pdop", "<f8")])
assert C.sizeof(FixConfig) == 56 and C.sizeof(FixPlan) == 32 and EPHEMERIS_DTYPE.itemsize == 200 and FIX_DTYPE.itemsize == 80


class ObsConfig(C.Structure):
    """gat_obs_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("format", C.c_int32), ("code_length", C.c_int32), ("symbol_blocks", C.c_int32),
                ("code_freq_nominal_hz", C.c_double), ("block_seconds", C.c_double), ("sampling_freq_hz", C.c_double), ("if_hz", C.c_double),
                ("block_samples", C.c_int32), ("max_frames", C.c_int32), ("min_tow_steps", C.c_int32), ("epoch_first", C.c_int32),
                ("epoch_stride", C.c_int32), ("rx_mode", C.c_int32), ("rx0_ms", C.c_int32), ("travel_ms", C.c_int32),
                ("edge_margin", C.c_double), ("rx0_frac", C.c_double)]


class ObsPlan(C.Structure):
    """gat_obs_plan (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("chunk_blocks", C.c_int32), ("num_chunks", C.c_int32), ("channel_group", C.c_int32),
                ("num_groups", C.c_int32), ("lanes", C.c_int32), ("rows", C.c_int32), ("run_blocks", C.c_int32), ("threads", C.c_int32),
                ("lds_bytes", C.c_int32), ("chunk_workgroups", C.c_int32), ("channel_workgroups", C.c_int32), ("scratch_bytes", C.c_int64)]


# gat_obs_channel (include/gat.h)
OBS_CHANNEL_DTYPE = np.dtype([("status", "<i4"), ("frame_block", "<i4"), ("tow_frame", "<i4"), ("frame0_ms", "<i4"), ("edge_period", "<i8"),
                              ("edge_fraction", "<f8")])
assert C.sizeof(ObsConfig) == 96 and C.sizeof(ObsPlan) == 56 and OBS_CHANNEL_DTYPE.itemsize == 32


class RaimConfig(C.Structure):
    """gat_raim_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("max_exclude", C.c_int32), ("trial_iter", C.c_int32), ("flags", C.c_uint32),
                ("threshold", C.c_double * (GAT_MAX_FIX_CHANNELS - 3))]


# gat_fix_integrity (include/gat.h)
INTEGRITY_DTYPE = np.dtype([("status", "<i4"), ("dof", "<i4"), ("num_excluded", "<i4"), ("excluded", "<i4", (4,)), ("reserved", "<i4"),
                            ("stat0", "<f8"), ("threshold0", "<f8"), ("stat", "<f8"), ("threshold", "<f8")])
assert C.sizeof(RaimConfig) == 504 and INTEGRITY_DTYPE.itemsize == 64


class VelConfig(C.Structure):
    """gat_vel_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("carrier_hz", C.c_double)]


# gat_velocity (include/gat.h)
VELOCITY_DTYPE = np.dtype([("status", "<i4"), ("num_valid", "<i4"), ("num_used", "<i4"), ("reserved", "<i4")]
                          + [(n, "<f8") for n in ("vx", "vy", "vz", "clock_drift", "rms_residual_mps", "ve", "vn", "vu", "sin_lat", "cos_lat",
                                                  "sin_lon", "cos_lon", "height_m")])
assert C.sizeof(VelConfig) == 16 and VELOCITY_DTYPE.itemsize == 120


class SnapConfig(C.Structure):
    """gat_snap_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("max_iter", C.c_int32), ("tol_m", C.c_double), ("mask_sin", C.c_double),
                ("init_xyz", C.c_double * 3), ("ambiguity_margin", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# gat_snap_fix (include/gat.h)
SNAP_FIX_DTYPE = np.dtype([("status", "<i4"), ("num_valid", "<i4"), ("num_used", "<i4"), ("iterations", "<i4")]
                          + [(n, "<f8") for n in ("x", "y", "z", "clock_bias_s", "coarse_time_s", "rms_residual_m", "last_step_m", "gdop", "pdop",
                                                  "tdop")])
assert C.sizeof(SnapConfig) == 64 and SNAP_FIX_DTYPE.itemsize == 96


class AtmConfig(C.Structure):
    """gat_atm_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("carrier_hz", C.c_double), ("floor_sin", C.c_double),
                ("alpha", C.c_double * 4), ("beta", C.c_double * 4), ("zenith_dry_m", C.c_double), ("zenith_wet_m", C.c_double)]


# gat_lnav_page18 (include/gat.h)
PAGE18_DTYPE = np.dtype([(n, "<i4") for n in ("valid", "data_id", "sv_id", "wnt", "dt_ls", "wnlsf", "dn", "dt_lsf")]
                        + [("alpha", "<f8", (4,)), ("beta", "<f8", (4,)), ("a0", "<f8"), ("a1", "<f8"), ("tot", "<f8")])
assert C.sizeof(AtmConfig) == 104 and PAGE18_DTYPE.itemsize == 120


class SmoothConfig(C.Structure):
    """gat_smooth_config (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("flags", C.c_uint32), ("window", C.c_int32), ("reserved", C.c_int32), ("carrier_hz", C.c_double),
                ("if_hz", C.c_double), ("epoch_seconds", C.c_double), ("cmc_gate_s", C.c_double), ("rate_gate_cycles", C.c_double)]


class SmoothPlan(C.Structure):
    """gat_smooth_plan (include/gat.h)."""

    _fields_ = [("struct_size", C.c_uint32), ("chunk_epochs", C.c_int32), ("num_chunks", C.c_int32), ("lanes", C.c_int32), ("rows", C.c_int32),
                ("run_epochs", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32), ("chunk_workgroups", C.c_int32),
                ("channel_workgroups", C.c_int32), ("output_workgroups", C.c_int32), ("reserved", C.c_int32), ("scratch_bytes", C.c_int64)]


# gat_smooth_channel (include/gat.h)
SMOOTH_CHANNEL_DTYPE = np.dtype([(n, "<i4") for n in ("measured", "arcs", "cmc_resets", "rate_resets")])
assert C.sizeof(SmoothConfig) == 56 and C.sizeof(SmoothPlan) == 56 and SMOOTH_CHANNEL_DTYPE.itemsize == 16


_LIB = None


def library_path() -> str:
    """Path of libgat.so; GAT_LIBRARY overrides it (kernel experiments: A/B builds)."""
    return os.environ.get("GAT_LIBRARY") or _build.LIB


def load(build_if_missing: bool = True):
    """Load libgat.so (building it with hipcc when absent/stale and hipcc is available)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if build_if_missing and not os.environ.get("GAT_LIBRARY") and _build.is_stale():
        try:
            _build.build_libgat()
        except Exception as exc:  # no hipcc on this machine
            if not os.path.exists(path):
                raise ImportError(f"libgat.so is not built and hipcc failed: {exc}") from exc
    if not os.path.exists(path):
        raise ImportError(f"{path} not found: run `python -m gpuacceleratedtracking_amd.build`")
    lib = C.CDLL(path)
    vp, i32, i64, u32, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint32, C.c_double
    pp = C.POINTER(ChannelParams)
    sp = C.POINTER(SignalDesc)
    i32p = C.POINTER(C.c_int32)
    sigs = {
        "gat_create": (i32, [i32, vp, C.POINTER(vp)]),
        "gat_destroy": (i32, [vp]),
        "gat_set_stream": (i32, [vp, vp]),
        "gat_sync": (i32, [vp]),
        "gat_last_error": (C.c_char_p, [vp]),
        "gat_version": (C.c_char_p, []),
        "gat_device_info": (i32, [vp, C.c_char_p, C.c_size_t, i32p, i32p]),
        "gat_set_codes": (i32, [vp, C.POINTER(C.c_int8), i32, i32]),
        "gat_gen_codes": (i32, [C.c_char_p, i32, C.POINTER(C.c_int8), i32p, C.POINTER(dbl)]),
        "gat_sample_shifts": (i32, [i32, dbl, dbl, dbl, i32p]),
        "gat_downconvert_and_correlate": (i32, [vp, sp, pp, i32, i32, i32, i32p, dbl, vp, vp, u32]),
        "gat_downconvert_and_correlate_dev": (i32, [vp, sp, vp, i32, i32, i32, i32p, dbl, vp, vp, u32]),
        "gat_gen_code_replica": (i32, [vp, vp, i64, i32, dbl, dbl, dbl, i64]),
        "gat_gen_code_replica_f32coord": (i32, [vp, vp, i64, i32, dbl, dbl, dbl, i64]),
        "gat_gen_signal": (i32, [vp, vp, vp, i32, i64, i32, i64, i64, i32, i32, vp, dbl, dbl]),
        "gat_reduce_cplx_multi": (i32, [vp, vp, vp, i64, i32, vp, vp]),
        "gat_tracking_update": (i32, [vp, vp, vp, i32, i32, C.POINTER(LoopConfig), vp, vp, vp]),
        "gat_tracking_run": (i32, [vp, C.POINTER(SignalDesc), i32, i32, i32, C.POINTER(C.c_int32), dbl,
                                   C.POINTER(LoopConfig), vp, vp, vp, vp, vp, i64, C.c_uint32, C.POINTER(C.c_int32)]),
        "gat_malloc": (i32, [vp, C.c_size_t, C.POINTER(vp)]),
        "gat_free": (i32, [vp, vp]),
        "gat_memcpy_h2d": (i32, [vp, vp, vp, C.c_size_t]),
        "gat_memcpy_d2h": (i32, [vp, vp, vp, C.c_size_t]),
        "gat_memset": (i32, [vp, vp, i32, C.c_size_t]),
        "gat_timer_start": (i32, [vp]),
        "gat_timer_stop": (i32, [vp, C.POINTER(C.c_float)]),
        "gat_last_launch_info": (i32, [vp, C.POINTER(LaunchInfo), C.c_size_t]),
        "gat_set_matrix_core": (i32, [vp, i32]),
        "gat_set_vector_tiling": (i32, [vp, i32, i32, i32]),
        "gat_set_option": (i32, [vp, C.c_char_p, i64]),
        "gat_gen_code_replica_multi": (i32, [vp, vp, i64, i64, i32, vp, dbl, i64]),
        "gat_downconvert_and_accumulate": (i32, [vp, sp, pp, i32, i32p, dbl, vp, vp, vp, vp, vp, vp]),
        "gat_gen_signal_noisy": (i32, [vp, vp, vp, i32, i64, i32, i64, i64, i32, i32, vp, dbl, dbl, vp, dbl, C.c_uint64]),
        "gat_device_count": (i32, [i32p]),
        "gat_memcpy_peer": (i32, [vp, vp, vp, vp, C.c_size_t]),
        "gat_group_create": (i32, [i32, i32p, C.POINTER(vp)]),
        "gat_group_destroy": (i32, [vp]),
        "gat_group_size": (i32, [vp, i32p]),
        "gat_group_ctx": (i32, [vp, i32, C.POINTER(vp)]),
        "gat_group_last_error": (C.c_char_p, [vp]),
        "gat_group_shard": (i32, [vp, i32, i32, i32p, i32p]),
        "gat_group_set_codes": (i32, [vp, C.POINTER(C.c_int8), i32, i32]),
        "gat_group_replicate": (i32, [vp, i32, C.POINTER(vp), C.c_size_t]),
        "gat_group_correlate": (i32, [vp, sp, pp, i32, i32, i32, i32p, dbl, C.POINTER(vp), C.POINTER(vp), u32]),
        "gat_group_gather": (i32, [vp, C.POINTER(vp), C.POINTER(vp), i32, i32, i32, i32, vp, vp]),
        "gat_group_sync": (i32, [vp]),
        "gat_resident_open": (i32, [vp, sp, i32, i32, i32p, dbl, C.POINTER(ResidentConfig), C.POINTER(vp)]),
        "gat_resident_correlate": (i32, [vp, pp, i64, vp, vp]),
        "gat_resident_info_get": (i32, [vp, C.POINTER(ResidentInfo), C.c_size_t]),
        "gat_resident_park": (i32, [vp]),
        "gat_resident_close": (i32, [vp]),
        "gat_tracking_update_host": (i32, [vp, vp, i32, i32, C.POINTER(LoopConfig), vp, vp, vp]),
        "gat_resident_tracking_run": (i32, [vp, i32, i64, i64, C.POINTER(LoopConfig), vp, vp, vp, vp, i64]),
        "gat_resident_park_all": (i32, [vp]),
        "gat_timer_lap": (i32, [vp]),
        "gat_timer_laps": (i32, [vp, C.POINTER(C.c_float), i32, i32p]),
        "gat_debug_read_stream": (i32, [vp, vp, C.c_size_t, i32, i32, C.POINTER(C.c_float)]),
        "gat_gen_code_replica_texaddr": (i32, [vp, vp, i64, i32, dbl, dbl, dbl, i64, i32, i32]),
        "gat_acquire": (i32, [vp, sp, i32, i32p, i32, dbl, C.POINTER(AcqConfig), vp, vp]),
        "gat_acq_stats_host": (i32, [vp, i32, i32, i32, C.POINTER(AcqConfig), dbl, i64, vp]),
        "gat_acquire_fft": (i32, [vp, sp, i32, i32p, i32, dbl, C.POINTER(AcqConfig), vp, vp]),
        "gat_acquire_fft_plan": (i32, [sp, i32, i32, dbl, C.POINTER(AcqConfig), i32, i32, i32, i32, i32, C.POINTER(AcqFftPlan)]),
        "gat_acquire_fft_host": (i32, [sp, i32, vp, i32, i32, i32p, i32, dbl, C.POINTER(AcqConfig), i32, i32, vp]),
        "gat_spatial_covariance": (i32, [vp, sp, i32, i32, vp, vp]),
        "gat_array_weights": (i32, [vp, vp, vp, i32, vp, vp, i32, i32, dbl, vp, vp]),
        "gat_array_weights_host": (i32, [vp, vp, i32, vp, vp, i32, i32, dbl, vp, vp]),
        "gat_beamform": (i32, [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
        "gat_beamform_samples": (i32, [vp, sp, i32, vp, vp, i32, sp]),
        "gat_condition_samples": (i32, [vp, sp, i32, vp, u32, sp, vp]),
        "gat_condition_samples_host": (i32, [sp, i32, vp, u32, sp, vp]),
        "gat_sample_stats": (i32, [vp, sp, i32, i32, vp, u32, vp]),
        "gat_agc_update": (i32, [vp, vp, i32, C.POINTER(AgcConfig), vp]),
        "gat_agc_update_host": (i32, [vp, i32, C.POINTER(AgcConfig), vp]),
        "gat_filter_samples": (i32, [vp, sp, i32, vp, vp, C.POINTER(FirConfig), sp]),
        "gat_filter_samples_host": (i32, [sp, i32, vp, vp, C.POINTER(FirConfig), sp]),
        "gat_sample_spectrum": (i32, [vp, sp, i32, vp, C.POINTER(SpectrumConfig), vp]),
        "gat_sample_spectrum_host": (i32, [sp, i32, vp, C.POINTER(SpectrumConfig), vp]),
        "gat_spacetime_covariance": (i32, [vp, sp, i32, i32, i32, vp, vp]),
        "gat_spacetime_filter": (i32, [vp, sp, i32, vp, vp, i32, i32, sp]),
        "gat_spacetime_filter_host": (i32, [sp, i32, vp, vp, i32, i32, sp]),
        "gat_track_monitor": (i32, [vp, vp, vp, i64, i32, i32, i32, C.POINTER(MonitorConfig), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gat_track_monitor_host": (i32, [vp, vp, i64, i32, i32, i32, C.POINTER(MonitorConfig), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]),
        "gat_track_monitor_plan": (i32, [i64, i32, i32, i32, C.POINTER(MonitorConfig), i32, i32, C.POINTER(MonitorPlan)]),
        "gat_accumulator_covariance": (i32, [vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp]),
        "gat_accumulator_covariance_host": (i32, [vp, vp, i64, i32, i32, i32, i32, i32, i32, vp, vp]),
        "gat_hermitian_eig": (i32, [vp, vp, vp, i32, i32, i32, u32, vp, vp, vp, vp]),
        "gat_hermitian_eig_host": (i32, [vp, vp, i32, i32, i32, u32, vp, vp, vp, vp]),
        "gat_subspace_plan": (i32, [i64, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(SubspacePlan)]),
        "gat_nav_decode": (i32, [vp, vp, vp, i32, C.POINTER(NavConfig), vp, vp, vp, vp]),
        "gat_nav_decode_host": (i32, [vp, vp, i32, C.POINTER(NavConfig), vp, vp, vp, vp]),
        "gat_nav_decode_plan": (i32, [i32, C.POINTER(NavConfig), C.POINTER(NavPlan)]),
        "gat_position_fix": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(FixConfig), vp, vp, vp, vp, vp]),
        "gat_position_fix_host": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(FixConfig), vp, vp, vp, vp, vp]),
        "gat_position_fix_plan": (i32, [i32, i32, C.POINTER(FixConfig), C.POINTER(FixPlan)]),
        "gat_lnav_ephemeris_host": (i32, [vp, i32, vp]),
        "gat_lnav_ephemeris_words_host": (i32, [vp, vp]),
        "gat_tracking_run_history": (i32, [vp, C.POINTER(SignalDesc), i32, i32, i32, C.POINTER(C.c_int32), dbl,
                                           C.POINTER(LoopConfig), vp, vp, vp, vp, i64, C.c_uint32, vp, vp]),
        "gat_observables": (i32, [vp, vp, vp, vp, vp, i32, i32, i32, C.POINTER(ObsConfig)] + [vp] * 9),
        "gat_observables_host": (i32, [vp, vp, vp, vp, i32, i32, i32, C.POINTER(ObsConfig)] + [vp] * 9),
        "gat_observables_plan": (i32, [i32, i32, i32, C.POINTER(ObsConfig), C.POINTER(ObsPlan)]),
        "gat_position_fix_raim": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(FixConfig), C.POINTER(RaimConfig)] + [vp] * 7),
        "gat_position_fix_raim_host": (i32, [vp, vp, vp, vp, vp, vp, i32, i32, C.POINTER(FixConfig), C.POINTER(RaimConfig)] + [vp] * 7),
        "gat_position_fix_raim_plan": (i32, [i32, i32, C.POINTER(FixConfig), C.POINTER(RaimConfig), C.POINTER(FixPlan)]),
        "gat_velocity_fix": (i32, [vp] * 8 + [i32, i32, C.POINTER(VelConfig), vp, vp, vp]),
        "gat_velocity_fix_host": (i32, [vp] * 7 + [i32, i32, C.POINTER(VelConfig), vp, vp, vp]),
        "gat_velocity_fix_plan": (i32, [i32, i32, C.POINTER(VelConfig), C.POINTER(FixPlan)]),
        "gat_range_corrections": (i32, [vp] * 8 + [i32, i32, C.POINTER(AtmConfig)] + [vp] * 5),
        "gat_range_corrections_host": (i32, [vp] * 7 + [i32, i32, C.POINTER(AtmConfig)] + [vp] * 5),
        "gat_range_corrections_plan": (i32, [i32, i32, C.POINTER(AtmConfig), C.POINTER(FixPlan)]),
        "gat_atm_atan2_host": (i32, [vp, vp, C.c_int64, vp]),
        "gat_smooth_observables": (i32, [vp] * 9 + [i32, i32, C.POINTER(SmoothConfig)] + [vp] * 5),
        "gat_smooth_observables_host": (i32, [vp] * 8 + [i32, i32, C.POINTER(SmoothConfig)] + [vp] * 5),
        "gat_smooth_observables_plan": (i32, [i32, i32, C.POINTER(SmoothConfig), C.POINTER(SmoothPlan)]),
        "gat_snapshot_fix": (i32, [vp] * 7 + [i32, i32, C.POINTER(SnapConfig)] + [vp] * 7),
        "gat_snapshot_fix_host": (i32, [vp] * 6 + [i32, i32, C.POINTER(SnapConfig)] + [vp] * 7),
        "gat_snapshot_fix_plan": (i32, [i32, i32, C.POINTER(SnapConfig), C.POINTER(FixPlan)]),
        "gat_lnav_page18_host": (i32, [vp, i32, vp]),
        "gat_lnav_page18_words_host": (i32, [vp, vp]),
        "gat_tracking_update_weighted": (i32, [vp, vp, vp, i32, i32, C.POINTER(LoopConfig), vp, vp, vp, vp, vp]),
        "gat_tracking_update_host_weighted": (i32, [vp, vp, i32, i32, C.POINTER(LoopConfig), vp, vp, vp, vp, vp]),
        "gat_tracking_run_weighted": (i32, [vp, C.POINTER(SignalDesc), i32, i32, i32, C.POINTER(C.c_int32), dbl,
                                            C.POINTER(LoopConfig), vp, vp, vp, vp, vp, i64, C.c_uint32, C.POINTER(C.c_int32), vp, vp]),
    }
    assert sorted(sigs) == sorted(EXPORTS)
    for name, (res, args) in sigs.items():
        if os.environ.get("GAT_LIBRARY") and not hasattr(lib, name):
            continue  # A/B against an OLDER development build that predates a symbol (GAT_LIBRARY override only)
        fn = getattr(lib, name)  # AttributeError if the symbol is missing: fail loudly
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib
