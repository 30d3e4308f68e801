"""CPU tests of the FFT acquisition search's host twin (include/gat.h gat_acquire_fft_host; the rule is csrc/gat_acq_fft.h) over the
whole accepted domain (tests/acqfft_ref.DOMAIN): every transform length 2^10 .. 2^18, the ends of the lag-segment geometry (N = F - 1,
N = 1, Jseg < s, J = 1), caller code tables of 1 .. 120 000 chips of any int8 value, first_shift at +-2^29 and on the phases where
the float-reciprocal modulo is one quotient off, padded antenna strides, overlapping blocks, offset views, negative Doppler steps
and carrier steps of half a cycle a sample and more -- the twin against the FP64 contract (tests/helpers.acq_power_oracle) on the
sampled bins of every Doppler row, at the project's RTOL.  This is the proof that the rule holds on every case; the device is
then held to the twin's bits (tests/test_acquisition_fft_domain_gpu.py).  Also: a unit-group count that does not divide the
units, and each refusal boundary from both sides, by the plan and by the twin."""
import ctypes as C

import numpy as np
import pytest

from tests import acqfft_ref as ref
from tests.helpers import RTOL

ARG, RANGE = 1, 2


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.mark.parametrize("name", list(ref.DOMAIN))
def test_twin_matches_oracle(g, name):
    """Worst (norm-wise / element-wise) errors over the Doppler rows and PRNs, in units of RTOL = 1e-5 (2026-10, this rule):
    A-2^10 0.005 / 0.009, A-2^11 0.009 / 0.009, A-2^12 0.005 / 0.005, A-2^13 0.012 / 0.012, A-2^14 0.028 / 0.061, A-2^15 0.019 / 0.024,
    A-2^16 0.085 / 0.085, A-2^17 0.063 / 0.063, A-2^18 0.053 / 0.127, B-seams-only 0.015 / 0.015, B-empty-segments 0.019 / 0.019,
    B-one-sample 0.029 / 0.035, B-one-bin 0.003 / 0.003, B-step-3 0.018 / 0.018, C-short-step-2^13 (and -batches; D = 18) 0.028 / 0.058,
    C-short-step-2^13-last (and -batches; D = 28) 0.028 / 0.069, C-short-step-2^12 (and -batches; D = 35) and C-short-step-2^12-last
    (and -batches; D = 56) 0.037 / 0.072, C-block-window 0.018 / 0.048, D-Lc1-int8 0.007 / 0.007, D-Lc2-ternary
    0.010 / 0.010, D-Lc257-int8 0.017 / 0.022, D-Lc257-zeros-2.5 0.018 / 0.019, D-Lc4092-ternary 0.030 / 0.033, D-Lc4092-int8-2.5
    0.015 / 0.045, D-Lc120000-int8 0.018 / 0.051, D-Lc120000-ternary 0.027 / 0.061, E-shift-+2^29 0.007 / 0.007, E-shift--2^29
    0.009 / 0.009, E-hard-pos-low 0.011 / 0.011, E-hard-neg-low 0.010 / 0.010, F-ant-stride 0.006 / 0.006, F-overlap 0.017 / 0.017,
    F-offset-cf32 0.006 / 0.006, F-offset-int16 0.009 / 0.009, F-offset-int8 0.013 / 0.013, F-negative-step 0.010 / 0.010,
    F-carrier-0.5fs 0.008 / 0.008, F-carrier-1.25fs 0.009 / 0.009, F-carrier--3.75fs 0.006 / 0.006.
    The work-split cases take the Doppler bin count the plan gives for 256 compute units; the twin itself runs with one group."""
    case = ref.DOMAIN[name]
    sc = ref.domain_scene(case)
    desc = ref.case_host_desc(g, case, sc)
    D = case.D if case.D > 0 else ref.short_step_doppler_bins(g, case, desc, 256)
    assert D is not None, "no Doppler bin count in 1 .. 64 leaves a short last step at 256 compute units"
    cfg = ref.case_config(g, case, D)
    pl = ref.plan(g, desc, case.B, len(case.prns), case.fs, cfg, case.log2)
    assert (pl["fft_log2"], pl["passes"], pl["num_segments"]) == (case.log2, *case.want), pl
    power = ref.twin(g, desc, case.B, case.prns, case.fs, cfg, case.log2, 1, sc["codes"])
    worst = ref.check_case(case, sc, power, D, case.log2, name)
    print(f"{name}: worst norm-wise {worst[0] / RTOL:.4f} RTOL, element-wise {worst[1] / RTOL:.4f} RTOL")


@pytest.mark.parametrize("name", ["C-short-step-2^13", "C-short-step-2^12"])
def test_twin_with_groups_that_do_not_divide_the_units(g, name):
    """Six units dealt to four groups (groups 0 and 1 own two units, 2 and 3 one), and to five: within RTOL of the contract, and
    not the bits of one group.  Worst errors in units of RTOL: 2^13 0.019 / 0.031 (4 groups), 0.023 / 0.032 (5); 2^12 0.014 / 0.014 (4),
    0.012 / 0.012 (5)."""
    case = ref.DOMAIN[name]
    sc = ref.domain_scene(case)
    desc = ref.case_host_desc(g, case, sc)
    D = 3
    cfg = ref.case_config(g, case, D)
    one = ref.twin(g, desc, case.B, case.prns, case.fs, cfg, case.log2, 1, sc["codes"])
    for groups in (4, 5):
        assert (case.M * case.B) % groups != 0
        power = ref.twin(g, desc, case.B, case.prns, case.fs, cfg, case.log2, groups, sc["codes"])
        worst = ref.check_case(case, sc, power, D, case.log2, f"{name}, {groups} groups")
        assert power.tobytes() != one.tobytes()
        print(f"{name}, {groups} groups: worst norm-wise {worst[0] / RTOL:.4f} RTOL, element-wise {worst[1] / RTOL:.4f} RTOL")


@pytest.mark.parametrize("name", list(ref.BOUNDARIES))
def test_refusal_boundaries(g, name):
    """The code just inside and just outside each bound, from gat_acquire_fft_plan and from the twin alike."""
    lib = g.load_library()
    for side, want in zip(ref.boundary_calls(name), (0, RANGE)):
        buf = np.zeros((1, side["N"] + 8), dtype=np.float32)
        buf[0, ::7] = 1.0
        desc = ref.host_desc(g, (buf, buf), ref.PLANAR, 1, side["N"], side["N"] + 8, side["N"])
        codes = ref.boundary_codes(side)
        cfg = ref.config(g, 1, side["J"], 1, side["first_shift"], 0.0, 0.0, 0.0, lc=codes.shape[1], fc=side["ratio"] * ref.FC)
        pl = g._lib.AcqFftPlan()
        pl.struct_size = C.sizeof(pl)
        rp = lib.gat_acquire_fft_plan(C.byref(desc), 1, 1, ref.FC, C.byref(cfg), side["log2"], 0, 0, 256, 0, C.byref(pl))
        out = np.zeros(side["J"], dtype=np.float32)
        prn = np.zeros(1, dtype=np.int32)
        rt = lib.gat_acquire_fft_host(C.byref(desc), 1, C.c_void_p(codes.ctypes.data), codes.shape[1], codes.shape[1],
                                      prn.ctypes.data_as(C.POINTER(C.c_int32)), 1, ref.FC, C.byref(cfg), side["twin_log2"], 1, C.c_void_p(out.ctypes.data))
        assert (rp, rt) == (want, want), (name, side, rp, rt)
        if want == 0:
            assert pl.fft_log2 == side["twin_log2"] and np.isfinite(out).all() and out.max() > 0
