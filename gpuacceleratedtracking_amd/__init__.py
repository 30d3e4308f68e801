"""gpuacceleratedtracking_amd -- MI355X-native GNSS tracking correlator.

Host-side mirror (Python) of the operator surface the reference (coezmaden/
GPUAcceleratedTracking + Tracking.jl) exposes for ONE path: downconvert + correlate.  All
compute runs in libgat.so (hand-written HIP for gfx950) through the C ABI of include/gat.h.
Importing this package never touches the test oracle and there is no CPU fallback: without the
HIP library / a HIP device the operators raise.
"""
from ._lib import GAT_FLAG_GRAPH, GAT_MC_AUTO, GAT_MC_BF16_SPLIT, GAT_MC_F32, GAT_MC_VECTOR  # noqa: F401
from ._lib import (GAT_FLAG_ATOMIC, GAT_LAYOUT_INTERLEAVED, GAT_LAYOUT_INTERLEAVED_I8,  # noqa: F401
                   GAT_LAYOUT_INTERLEAVED_I16, GAT_LAYOUT_PLANAR, SAMPLE_BYTES, GatError,
                   library_path, load as load_library)
from .acquisition import AcquisitionResult, acquire, acquire_fft_host, acquire_fft_plan, acquisition_stats_host, tracking_init  # noqa: F401
from .algorithms import (ALGODICT, ALGODICTINV, MEMDICT, REDDICT, KernelAlgorithm, ReductionAlgorithm,  # noqa: F401
                         ReplicaAlgorithm, cpu_reduce_partial_sum, cuda_reduce_partial_sum, kernel_algorithm)
from .array import (GAT_BF_CONVENTIONAL, GAT_BF_MVDR, GAT_BF_POWER_INVERSION, beamform, beamform_samples,  # noqa: F401
                    beamformer_weights, spatial_covariance)
from .atmosphere import (Klobuchar, Page18, RangeCorrections, atmosphere_plan, lnav_page18, lnav_page18_payload,  # noqa: F401
                         position_fix_corrected, range_corrections, range_corrections_host, tropo_zenith, tropo_zenith_from_fix)
from .benchmarks import (add_metadata, add_results, algorithmic_bytes, build_stream,  # noqa: F401
                         run_kernel_benchmark, run_reduction_benchmark, run_replica_benchmark, stream_scenario)
from .context import Context, ResidentCorrelator, get_context  # noqa: F401
from .correlator import (EarlyPromptLateCorrelator, NumAccumulators, NumAnts, get_accumulators,  # noqa: F401
                         get_correlator_sample_shifts, get_num_accumulators, get_num_ants)
from .frontend import (GAT_COND_BLANK_ALL_ANTS, SampleStats, agc_params, agc_params_host, condition_samples,  # noqa: F401
                       condition_samples_host, requantize, sample_stats)
from .filtering import (channelize, filter_samples, filter_samples_host, filter_stream, lowpass_taps, notch_taps,  # noqa: F401
                        shift_taps)
from .gen_signal import StructSignal, gen_blank_signal, gen_signal, gen_signal_stream, make_params  # noqa: F401
from .loop import ResidentTrackingLoop, TrackingLoop  # noqa: F401
from .monitor import (TrackMonitor, monitor_accumulators, monitor_accumulators_host, monitor_plan, overlay_for)  # noqa: F401
from .navigation import (NavResult, cnav_fec_encode, cnav_message, crc24q, decode_navigation, decode_navigation_host,  # noqa: F401
                         lnav_subframe, nav_format_for, nav_plan)
from .observables import Observables, obs_config, observables, observables_host, observables_plan  # noqa: F401
from .positioning import (Ephemeris, PositionFix, lnav_ephemerides, lnav_ephemeris, lnav_ephemeris_payloads, position_fix,  # noqa: F401
                          position_fix_host, position_fix_raim, position_fix_raim_host, position_plan, raim_config, raim_plan,
                          raim_thresholds)
from .sharding import DeviceGroup, ShardPlan, gather_outputs, shard_channels, shard_params  # noqa: F401
from .spectrum import (auto_notch, find_tones, sample_spectrum, sample_spectrum_host, spectrum_stream)  # noqa: F401
from .spacetime import (spacetime_covariance, spacetime_delay, spacetime_filter, spacetime_filter_host, spacetime_steering,  # noqa: F401
                        spacetime_stream, spacetime_weights)
from .smoothing import SmoothedObservables, smooth_observables, smooth_observables_host, smoothing_plan  # noqa: F401
from .snapshot import SnapshotFix, code_fractions, snapshot_fix, snapshot_fix_host, snapshot_plan  # noqa: F401
from .signals import GNSSDICT, GPSL1, GPSL5, generate_codes, get_code_frequency, get_code_length  # noqa: F401
from .subspace import (accumulator_covariance, accumulator_covariance_host, hermitian_eig, hermitian_eig_host, source_count,  # noqa: F401
                       steering_from_accumulators, subspace_plan)
from .velocity import VelocityFix, velocity_fix, velocity_fix_host, velocity_plan  # noqa: F401
from .tracking import (StreamCorrelator, downconvert_and_accumulate_strided, downconvert_and_correlate,  # noqa: F401
                       gen_code_replica, gen_code_replica_nsat, reduce_cplx_multi)

__version__ = "0.1.0"
