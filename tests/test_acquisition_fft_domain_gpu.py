"""GPU tests of the FFT acquisition search (include/gat.h gat_acquire_fft, csrc/gat_acq_fft.hip) over its whole accepted domain and
work split (tests/acqfft_ref.DOMAIN; tests/test_acquisition_fft_domain_host.py holds the twin to the FP64 contract on the same
cases): every case runs through the raw call into a grid pre-filled with -1 and must equal the host twin bit for bit at the
plan's transform length and unit-group count, and lie within RTOL of the contract on the sampled bins of every Doppler row.
A. every transform length 2^10 .. 2^18: both one-pass lengths' ends, and all six (L1, L2) pairs of the two passes;
B. the ends of the lag-segment geometry (N = F - 1, N = 1, Jseg < s, J = 1, s = 3 across seams);
C. unit counts that are no multiple of the group count, alone and with unit batches (the short last step), a moving block window,
   and power_dev = NULL;
D. caller code tables of 1 .. 120 000 chips (padded row stride, unsorted and repeated rows, several chips a sample);
E. first_shift at +-2^29 and on the phases where the float-reciprocal modulo is one quotient off;
F. padded antenna strides, overlapping blocks, offset views, negative Doppler steps, carrier steps of half a cycle and more.
Then each refusal boundary from both sides, by the device call."""
import ctypes as C

import numpy as np
import pytest

from tests import acqfft_ref as ref
from tests.helpers import RTOL, standard_codes_after  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

OPTIONS = ("acq_fft_log2", "acq_fft_doppler_batch", "acq_fft_unit_batch")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture()
def ctx(g, standard_codes_after):  # noqa: F811
    c = g.get_context()
    yield c
    for name in OPTIONS:
        c.set_option(name, 0)


def _device_desc(case, sc):
    """The case's buffers on the device and the descriptor of the view `offset` elements into them."""
    import torch
    from gpuacceleratedtracking_amd.tracking import _signal_desc
    t = tuple(torch.from_numpy(a).cuda() for a in sc["arrays"])
    desc = _signal_desc(t[0], t[1] if case.layout == ref.PLANAR else None, case.N, start=case.offset, block_stride=case.block_stride)
    assert desc.ant_stride == sc["row"] and desc.num_ants == case.M
    return t, desc


def _call(g, ctx, desc, B, prns, fs, cfg, keep_power=True):
    """The raw call: (status, grid [P, D, J] on the host or None, results)."""
    import torch
    P = len(prns)
    power = torch.full((P, cfg.num_doppler_bins, cfg.num_code_bins), -1.0, dtype=torch.float32, device="cuda") if keep_power else None
    res = np.zeros(P, dtype=g._lib.ACQ_RESULT_DTYPE)
    pr = np.ascontiguousarray(prns, dtype=np.int32)
    rc = ctx.lib.gat_acquire_fft(ctx._h, C.byref(desc), B, pr.ctypes.data_as(C.POINTER(C.c_int32)), P, fs, C.byref(cfg),
                                 C.c_void_p(power.data_ptr()) if keep_power else None, C.c_void_p(res.ctypes.data))
    return rc, power.cpu().numpy() if keep_power else None, res


def _prepare(g, ctx, case):
    """The scene, the host descriptor, the Doppler bin count, the configuration and the device's plan, with the options set."""
    sc = ref.domain_scene(case)
    hdesc = ref.case_host_desc(g, case, sc)
    cus = ctx.device_info()["num_cus"]
    D = case.D if case.D > 0 else ref.short_step_doppler_bins(g, case, hdesc, cus)
    assert D is not None, f"no Doppler bin count in 1 .. 64 leaves a short last step at {cus} compute units"
    cfg = ref.case_config(g, case, D)
    P, units = len(case.prns), case.M * case.B
    pl = ref.plan(g, hdesc, case.B, P, case.fs, cfg, case.log2, cus)
    ubatch = pl["unit_groups"] if case.ubatch < 0 else case.ubatch
    pl = ref.plan(g, hdesc, case.B, P, case.fs, cfg, case.log2, cus, ubatch=ubatch)
    assert (pl["fft_log2"], pl["passes"], pl["num_segments"]) == (case.log2, *case.want), pl
    if case.D <= 0:
        assert units % pl["unit_groups"] != 0, pl  # the call's last step is short
    if case.ubatch < 0:
        assert pl["unit_batch"] == pl["unit_groups"] < units, pl  # one step a batch; the last batch holds the short step
    if case.ubatch > 0:
        assert pl["unit_batch"] < units and pl["unit_batch"] % case.M != 0, pl  # the block window moves, a block lies in two batches
    ctx.set_codes(sc["codes"])
    ctx.set_option("acq_fft_log2", case.log2)
    ctx.set_option("acq_fft_unit_batch", ubatch)
    return sc, hdesc, D, cfg, pl


@pytest.mark.parametrize("name", list(ref.DOMAIN))
def test_device_equals_twin_and_matches_oracle(g, ctx, name):
    case = ref.DOMAIN[name]
    sc, hdesc, D, cfg, pl = _prepare(g, ctx, case)
    keep, desc = _device_desc(case, sc)
    rc, power, _ = _call(g, ctx, desc, case.B, case.prns, case.fs, cfg)
    assert rc == 0, ctx.lib.gat_last_error(ctx._h)
    units = case.M * case.B
    print(f"{name}: log2 F {pl['fft_log2']}, passes {pl['passes']}, segments {pl['num_segments']}, groups {pl['unit_groups']}, units {units}, "
          f"unit batches {-(-units // pl['unit_batch'])}, Doppler bins {D} in batches of {pl['doppler_batch']}")
    twin = ref.twin(g, hdesc, case.B, case.prns, case.fs, cfg, pl["fft_log2"], pl["unit_groups"], sc["codes"])
    assert power.tobytes() == twin.tobytes(), f"{name}: {np.count_nonzero(power != twin)} of {power.size} bins differ, worst {np.abs(power - twin).max() / twin.max():.3e}"
    worst = ref.check_case(case, sc, power, D, pl["fft_log2"], name)
    print(f"{name}: worst norm-wise {worst[0] / RTOL:.4f} RTOL, element-wise {worst[1] / RTOL:.4f} RTOL")


@pytest.mark.parametrize("name", ["C-short-step-2^13-last", "C-short-step-2^12-batches"])
def test_results_without_a_caller_grid(g, ctx, name):
    """power_dev = NULL (the grid stays in the scratch, which the plan carves differently): the same results, byte for byte."""
    case = ref.DOMAIN[name]
    sc, hdesc, D, cfg, pl = _prepare(g, ctx, case)
    keep, desc = _device_desc(case, sc)
    rc1, power, with_grid = _call(g, ctx, desc, case.B, case.prns, case.fs, cfg)
    rc2, _, without = _call(g, ctx, desc, case.B, case.prns, case.fs, cfg, keep_power=False)
    assert rc1 == 0 and rc2 == 0, ctx.lib.gat_last_error(ctx._h)
    assert with_grid.tobytes() == without.tobytes()
    h = g.acquisition_stats_host(power, cfg, case.fs, case.N)
    for f in ("detected", "doppler_bin", "code_bin", "num_noise_bins"):
        assert np.array_equal(h[f], with_grid[f]), f
    assert np.array_equal(with_grid["prn"], case.prns)


@pytest.mark.parametrize("name", list(ref.BOUNDARIES))
def test_refusal_boundaries(g, ctx, name):
    """The code just inside and just outside each bound, as tests/test_acquisition_fft_domain_host.py has it for the plan and the twin."""
    import torch
    from gpuacceleratedtracking_amd.tracking import _signal_desc
    for side, want in zip(ref.boundary_calls(name), (0, 2)):
        re = torch.zeros((1, side["N"] + 8), dtype=torch.float32, device="cuda")
        re[0, ::7] = 1.0
        desc = _signal_desc(re, re, side["N"])
        codes = ref.boundary_codes(side)
        ctx.set_codes(codes)
        ctx.set_option("acq_fft_log2", side["log2"])
        cfg = ref.config(g, 1, side["J"], 1, side["first_shift"], 0.0, 0.0, 0.0, lc=codes.shape[1], fc=side["ratio"] * ref.FC)
        rc, power, _ = _call(g, ctx, desc, 1, [0], ref.FC, cfg)
        assert rc == want, (name, side, rc, ctx.lib.gat_last_error(ctx._h))
        if want == 0:
            hbuf = re.cpu().numpy()
            twin = ref.twin(g, ref.host_desc(g, (hbuf, hbuf), ref.PLANAR, 1, side["N"], side["N"] + 8, side["N"]), 1, [0], ref.FC, cfg, side["twin_log2"], 1, codes)
            assert power.tobytes() == twin.tobytes()
        else:
            assert (power == -1.0).all()  # a refused call writes nothing
