"""The Python layer's result and plan rules (gpuacceleratedtracking_amd/results.py) on the CPU, without the library: the keys every
plan function reports, the choice of optional outputs, the one synchronisation and the record views of a result, and the refusal
of a call without a context."""
import numpy as np
import pytest

from gpuacceleratedtracking_amd import _lib, results

# what each plan function returned before results.py stated the rule once: the struct's fields without struct_size and reserved
PLAN_KEYS = {
    "monitor_plan": ("MonitorPlan", ["num_windows", "search_symbols", "symbol_capacity", "prompt_workgroups", "window_workgroups", "term_workgroups",
                                     "energy_workgroups", "pick_workgroups", "symbol_workgroups", "scratch_bytes"]),
    "nav_plan": ("NavPlan", ["num_phases", "bit_capacity", "num_candidates", "slice_workgroups", "quantise_workgroups", "trellis_workgroups",
                             "score_workgroups", "pick_workgroups", "frame_workgroups", "scratch_bytes"]),
    "observables_plan": ("ObsPlan", ["chunk_blocks", "num_chunks", "channel_group", "num_groups", "lanes", "rows", "run_blocks", "threads", "lds_bytes",
                                     "chunk_workgroups", "channel_workgroups", "scratch_bytes"]),
    "position_plan": ("FixPlan", ["workgroups", "waves_per_workgroup", "threads", "lds_bytes", "scratch_bytes"]),
    "raim_plan": ("FixPlan", ["workgroups", "waves_per_workgroup", "threads", "lds_bytes", "scratch_bytes"]),
    "subspace_plan": ("SubspacePlan", ["num_estimates", "chunks_per_estimate", "cov_split", "cov_workgroups", "cov_threads", "cov_lds_bytes",
                                       "cov_reduce_workgroups", "eig_workgroups", "eig_threads", "eig_lds_bytes", "scratch_bytes"]),
    "acquire_fft_plan": ("AcqFftPlan", ["fft_log2", "num_segments", "segment_lags", "passes", "doppler_batch", "unit_batch", "unit_groups",
                                        "scratch_bytes"]),
}


@pytest.mark.parametrize("function", sorted(PLAN_KEYS))
def test_plan_report_keeps_every_plan_functions_keys(function):
    import ctypes

    struct, keys = PLAN_KEYS[function]
    cls = getattr(_lib, struct)
    plan = results.new_plan(cls)
    assert plan.struct_size == ctypes.sizeof(cls)
    for i, name in enumerate(keys):
        setattr(plan, name, i + 1)
    report = results.plan_report(plan)
    assert list(report) == keys and list(report.values()) == list(range(1, len(keys) + 1))
    assert all(type(v) is int for v in report.values())


def test_wanted_refuses_unknown_names_and_none_is_the_default():
    known = ("sat", "resid", "sin_el", "used", "trial")
    assert results.wanted(None, known, known[:4]) == known[:4]
    assert results.wanted(["trial", "sat"], known, known[:4]) == ("trial", "sat")
    assert results.wanted((), known, known) == ()
    with pytest.raises(ValueError) as e:
        results.wanted(("sat", "zeta", "alpha"), known, known)
    assert str(e.value) == f"unknown outputs ['alpha', 'zeta']: choose from {known}"


class CountingContext:
    def __init__(self):
        self.syncs = 0

    def sync(self):
        self.syncs += 1


def test_result_synchronises_once_and_views_the_record_buffers():
    window = np.dtype([("sum", "<f8"), ("blocks", "<i8")])
    channel = np.dtype([("start", "<i4"), ("count", "<i4")])

    class Result(results.PlannedResult):
        _VIEWS = {"windows": (window, True), "channels": (channel, False)}

    K, NW = 3, 5
    raw = {"windows": np.arange(K * NW * 2, dtype=np.float64).reshape(K, NW * 2),  # as a device call allocates: plain words
           "channels": np.arange(K * 2, dtype=np.int32).reshape(K, 2),
           "energy": np.ones((K, 7))}
    ctx = CountingContext()
    r = Result(raw, ctx)
    assert r._raw is raw and r._ctx is ctx and r._host is None and ctx.syncs == 0
    for _ in range(3):
        h = r._h()
        assert h["windows"].dtype == window and h["windows"].shape == (K, NW)
        assert h["channels"].dtype == channel and h["channels"].shape == (K,)
        assert h["energy"] is raw["energy"]
    assert ctx.syncs == 1 and r._h() is h
    assert h["windows"]["sum"][1, 2] == raw["windows"][1, 4] and h["channels"]["count"].tolist() == [1, 3, 5]
    # a host twin's arrays are structured already and there is no context
    twin = Result({"windows": np.zeros((K, NW), dtype=window), "channels": np.zeros(K, dtype=channel)})
    assert twin._ctx is None and twin._h()["windows"].shape == (K, NW) and twin._h()["channels"].shape == (K,)


def test_the_four_results_share_the_base_and_keep_their_views():
    from gpuacceleratedtracking_amd.monitor import TrackMonitor
    from gpuacceleratedtracking_amd.navigation import NavResult
    from gpuacceleratedtracking_amd.observables import Observables
    from gpuacceleratedtracking_amd.positioning import PositionFix

    for cls, views in ((TrackMonitor, {"windows": (_lib.MONITOR_WINDOW_DTYPE, True), "channels": (_lib.MONITOR_CHANNEL_DTYPE, False)}),
                       (NavResult, {"channels": (_lib.NAV_CHANNEL_DTYPE, False), "frames": (_lib.NAV_FRAME_DTYPE, True)}),
                       (Observables, {"channels": (_lib.OBS_CHANNEL_DTYPE, False)}),
                       (PositionFix, {"fixes": (_lib.FIX_DTYPE, False), "integrity": (_lib.INTEGRITY_DTYPE, False)})):
        assert issubclass(cls, results.PlannedResult) and cls._VIEWS == views and "_h" not in vars(cls)
    ctx = CountingContext()
    E, K = 4, 6
    fix = PositionFix({"fixes": np.zeros((E, _lib.FIX_DTYPE.itemsize), dtype=np.uint8), "sat": np.zeros((E, K, 4))}, ctx)
    assert fix.status.shape == (E,) and fix.xyz.shape == (E, 3) and fix.ok.all() and fix.sat.shape == (E, K, 4) and ctx.syncs == 1
    with pytest.raises(AttributeError, match="resid was not asked for"):
        fix.resid


def test_host_check_raises_the_code_and_the_name():
    assert results.host_check(0, "gat_position_fix_host") is None
    with pytest.raises(_lib.GatError) as e:
        results.host_check(2, "gat_position_fix_host")
    assert e.value.status == 2 and str(e.value) == "gat_position_fix_host: GAT_ERR_RANGE"
