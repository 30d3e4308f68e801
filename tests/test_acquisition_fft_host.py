"""CPU tests of the FFT acquisition search's host twin (include/gat.h gat_acquire_fft_host, gat_acquire_fft_plan; the rule is
csrc/gat_acq_fft.h): the twin against the FP64 contract (tests/helpers.acq_power_oracle) at the shapes that reach every instance
-- one pass, two passes, several lag segments, odd N, block_stride != N, negative first_shift, s > 1, several antennas and blocks,
integer samples --, every bin of one small grid, the invariances (a Doppler row does not depend on the rows searched with it; the
transform length and the unit-group count move a bin by rounding only) and every refusal, which the plan reports as the call does."""
import ctypes as C

import numpy as np
import pytest

import oracle
from tests import acqfft_ref as ref
from tests.helpers import RTOL, acq_power_oracle, check_power_close


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def _run(g, name, log2=None, groups=1, rows=None):
    layout, M, B, N, bstride, fs, s, first_shift, J, D, if_hz, lg = ref.SHAPES[name]
    ld = ref.length(B, N, bstride)
    arrays, re, im = ref.scene(100 + layout, layout, M, ld, fs, if_hz)
    desc = ref.host_desc(g, arrays, layout, M, N, ld, bstride)
    f_first = ref.F_FIRST if rows is None else ref.F_FIRST + rows[0] * ref.F_STEP
    cfg = ref.config(g, D if rows is None else len(rows), J, s, first_shift, f_first, ref.F_STEP, if_hz)
    pl = ref.plan(g, desc, B, len(ref.PRNS), fs, cfg, log2 if log2 is not None else lg)
    power = ref.twin(g, desc, B, ref.PRNS, fs, cfg, pl["fft_log2"], groups)
    return power, pl, (re, im, cfg, arrays)


@pytest.mark.parametrize("name", list(ref.SHAPES))
def test_twin_matches_oracle(g, name):
    """Worst (norm-wise, element-wise) errors per Doppler row, in units of RTOL = 1e-5 (2026-10, this rule):
    one-pass 0.041 / 0.117, two-pass-two-segments 0.031 / 0.109, odd-blocks 0.024 / 0.058, int16 0.029 / 0.057, int8 0.027 / 0.071."""
    layout, M, B, N, bstride, fs, s, first_shift, J, D, if_hz, _ = ref.SHAPES[name]
    power, pl, (re, im, cfg, _) = _run(g, name)
    want = {"one-pass": (12, 1, 1), "two-pass-two-segments": (13, 2, 2), "odd-blocks": (13, 2, 1), "int16": (12, 1, 1), "int8": (12, 1, 3)}[name]
    assert (pl["fft_log2"], pl["passes"], pl["num_segments"]) == want, pl
    rng = np.random.default_rng(7)
    codes = oracle.codes("GPSL1", 32)
    rows = np.arange(D)
    worst = [0.0, 0.0]
    for pi, p in enumerate(ref.PRNS):
        peak = np.unravel_index(np.argmax(power[pi]), power[pi].shape)
        jsel = ref.sample_bins(rng, J, s, N, pl["fft_log2"], extra=[peak[1]])
        want_p = acq_power_oracle(re, im, codes, p, ref.FC, ref.LC, fs, if_hz, ref.F_FIRST, ref.F_STEP, rows, first_shift, s, jsel, N, B, bstride)
        e = check_power_close(power[pi][:, jsel], want_p, what=f"{name} prn {p}")
        worst = [max(worst[0], e[0]), max(worst[1], e[1])]
    print(f"{name}: worst norm-wise {worst[0] / RTOL:.4f} RTOL, element-wise {worst[1] / RTOL:.4f} RTOL")


def test_twin_every_bin_of_a_small_grid(g):
    """N = 700 in F = 1024 (Jseg = 325), J = 800 at s = 1: three segments, two antennas, two blocks that do not abut, first_shift
    < 0 -- every bin of the grid against the contract."""
    M, B, N, bstride, fs, J, D, first_shift = 2, 2, 700, 733, 2.046e6, 800, 3, -11
    ld = ref.length(B, N, bstride)
    arrays, re, im = ref.scene(5, ref.PLANAR, M, ld, fs, 0.0)
    desc = ref.host_desc(g, arrays, ref.PLANAR, M, N, ld, bstride)
    cfg = ref.config(g, D, J, 1, first_shift, -250.0, 250.0)
    pl = ref.plan(g, desc, B, len(ref.PRNS), fs, cfg, 10)
    assert (pl["fft_log2"], pl["passes"], pl["num_segments"], pl["segment_lags"]) == (10, 1, 3, 325)
    power = ref.twin(g, desc, B, ref.PRNS, fs, cfg, 10)
    codes = oracle.codes("GPSL1", 32)
    for pi, p in enumerate(ref.PRNS):
        want = acq_power_oracle(re, im, codes, p, ref.FC, ref.LC, fs, 0.0, -250.0, 250.0, np.arange(D), first_shift, 1, np.arange(J), N, B, bstride)
        e = check_power_close(power[pi], want, what=f"prn {p}")
        print(f"every bin, prn {p}: norm-wise {e[0] / RTOL:.4f} RTOL, element-wise {e[1] / RTOL:.4f} RTOL")


def test_a_row_does_not_depend_on_the_rows_around_it(g):
    """The Doppler rows 2 .. 4 searched alone equal those rows of the whole search bit for bit (what lets the device batch the axis)."""
    whole, _, _ = _run(g, "int16")
    part, _, _ = _run(g, "int16", rows=[2, 3, 4])
    assert part.tobytes() == np.ascontiguousarray(whole[:, 2:5]).tobytes()


def _rows_close(a, b, what):
    a, b = a.astype(np.float64), b.astype(np.float64)
    for p in range(a.shape[0]):
        for i in range(a.shape[1]):
            e = np.abs(a[p, i] - b[p, i]).max() / b[p, i].max()
            assert e <= 2 * RTOL, f"{what} prn row {p} Doppler row {i}: {e:.3e}"


def test_transform_length_and_groups_move_bins_by_rounding_only(g):
    """Each F and each group count is within RTOL of the truth, so two of them agree within 2 RTOL norm-wise per row; and they do
    differ in bits (the parameters are not ignored)."""
    base, pl, _ = _run(g, "odd-blocks")
    assert pl["fft_log2"] == 13
    other, pl14, _ = _run(g, "odd-blocks", log2=14)
    assert pl14["fft_log2"] == 14 and pl14["passes"] == 2
    _rows_close(other, base, "F = 2^14 against 2^13")
    assert other.tobytes() != base.tobytes()
    for groups in (2, 3):  # (six groups of one unit each add in unit order again)
        grp, _, _ = _run(g, "odd-blocks", groups=groups)
        _rows_close(grp, base, f"{groups} unit groups against 1")
        assert grp.tobytes() != base.tobytes()
    small, pl12, _ = _run(g, "int16", log2=12)
    big, pl13, _ = _run(g, "int16", log2=13)
    assert (pl12["passes"], pl13["passes"]) == (1, 2)
    _rows_close(big, small, "two passes (2^13) against one (2^12)")


def test_refusals(g):
    """Every refusal returns its code, from the plan and from the twin alike."""
    lib = g.load_library()
    M, B, N, fs = 2, 2, 1500, 2.0e6
    ld = ref.length(B, N, N)
    arrays, _, _ = ref.scene(1, ref.PLANAR, M, ld, fs, 0.0, noise=0.1)
    codes = np.ascontiguousarray(oracle.codes("GPSL1", 32))
    prn = np.array([3], dtype=np.int32)
    out = np.zeros(5 * 400, dtype=np.float32)

    def both(desc=None, B_=B, cfg=None, log2=11, P=1, groups=1):
        d = desc if desc is not None else ref.host_desc(g, arrays, ref.PLANAR, M, N, ld, N)
        c = cfg if cfg is not None else ref.config(g, 5, 400, 1)
        pl = g._lib.AcqFftPlan()
        pl.struct_size = C.sizeof(pl)
        rp = lib.gat_acquire_fft_plan(C.byref(d), B_, P, fs, C.byref(c), log2, 0, 0, 256, 0, C.byref(pl))
        rt = lib.gat_acquire_fft_host(C.byref(d), B_, C.c_void_p(codes.ctypes.data), ref.LC, ref.LC, prn.ctypes.data_as(C.POINTER(C.c_int32)), P, fs,
                                      C.byref(c), log2, groups, C.c_void_p(out.ctypes.data))
        return rp, rt

    ARG, RANGE = 1, 2
    assert both() == (0, 0)
    assert both(cfg=ref.config(g, 0, 400, 1)) == (ARG, ARG)         # empty grid
    assert both(cfg=ref.config(g, 5, 0, 1)) == (ARG, ARG)
    assert both(P=0) == (ARG, ARG)
    assert both(cfg=ref.config(g, 5, 400, 0)) == (ARG, ARG)         # s < 1
    assert both(cfg=ref.config(g, 5, 400, 40)) == (RANGE, RANGE)    # s above the bound
    assert both(cfg=ref.config(g, 4096, 20000, 1)) == (RANGE, RANGE)  # grid above 2^26 bins
    c = ref.config(g, 5, 400, 1)
    c.reserved = 1
    assert both(cfg=c) == (ARG, ARG)
    c = ref.config(g, 5, 400, 1)
    c.struct_size = 8
    assert both(cfg=c) == (ARG, ARG)
    c = ref.config(g, 5, 400, 1)
    c.code_freq_hz = 0.0
    assert both(cfg=c) == (ARG, ARG)
    assert both(cfg=ref.config(g, 5, 400, 1, f_step=1e13)) == (RANGE, RANGE)  # carrier out of range
    assert both(B_=0) == (ARG, ARG)
    d = ref.host_desc(g, arrays, ref.PLANAR, M, N, ld, N)
    d.chan_stride = 8
    assert both(desc=d) == (ARG, ARG)                               # chan_stride, as gat_acquire answers it
    d = ref.host_desc(g, arrays, ref.PLANAR, M, N, ld, N)
    d.layout = 7
    assert both(desc=d) == (ARG, ARG)
    d = ref.host_desc(g, arrays, ref.PLANAR, M, N, ld, N)
    d.num_samples = 1 << 18
    assert both(desc=d, log2=0)[0] == RANGE                         # N too long for the largest transform
    assert both(desc=d, log2=18) == (RANGE, RANGE)
    assert both(log2=10) == (RANGE, RANGE)                          # forced F = 1024 <= N
    assert both(log2=9) == (RANGE, RANGE) and both(log2=19) == (RANGE, RANGE)
    assert both(cfg=ref.config(g, 5, 400, 1, first_shift=1 << 30)) == (RANGE, RANGE)  # span
    assert both(groups=M * B)[1] == 0 and both(groups=M * B + 1)[1] == ARG and both(groups=0)[1] == ARG
    assert both(log2=0)[0] == 0 and both(log2=0)[1] == ARG          # the twin takes the transform length as given
    # a search whose spectra cannot fit 1 GiB at the smallest batches: N = 4095 forced into F = 4096 leaves two lags a segment
    d = ref.host_desc(g, arrays, ref.PLANAR, 1, 1023, ld, N)
    assert both(desc=d, B_=1, cfg=ref.config(g, 1, 1 << 20, 31), log2=10, P=32)[0] == RANGE
    pl = g._lib.AcqFftPlan()
    assert lib.gat_acquire_fft_plan(C.byref(d), 1, 1, fs, C.byref(ref.config(g, 5, 400, 1)), 0, 0, 0, 256, 0, C.byref(pl)) == ARG  # struct_size
    assert lib.gat_acquire_fft_plan(None, 1, 1, fs, C.byref(ref.config(g, 5, 400, 1)), 0, 0, 0, 256, 0, None) == ARG


def test_plan_report(g):
    """The default GPS L1 grid: F = 32768 in two passes, two lag segments at s = 10 and at s = 1; the batches fit the scratch."""
    fs, N, M = 20.0e6, 20000, 4
    buf = np.zeros((M, N + 8), dtype=np.float32)
    desc = ref.host_desc(g, (buf, buf), ref.PLANAR, M, N, N + 8, N)
    for s, J in ((10, 2000), (1, 20000)):
        pl = ref.plan(g, desc, 1, 32, fs, ref.config(g, 29, J, s, f_first=-7000.0, f_step=500.0), num_cus=256)
        assert (pl["fft_log2"], pl["passes"], pl["num_segments"], pl["segment_lags"], pl["unit_groups"]) == (15, 2, 2, 12769, 1), pl
        assert 1 <= pl["doppler_batch"] <= 29 and pl["unit_batch"] == 4 and pl["scratch_bytes"] <= 1 << 30, pl
    # one PRN, one Doppler bin: the units are dealt to groups; forced batches are reported as the call would use them
    pl = ref.plan(g, desc, 1, 1, fs, ref.config(g, 1, 2000, 10, f_first=0.0, f_step=0.0), num_cus=256)
    assert pl["unit_groups"] == 4 and pl["unit_batch"] == 4, pl
    pl = ref.plan(g, desc, 1, 4, fs, ref.config(g, 29, 2000, 10, f_first=-7000.0, f_step=500.0), num_cus=8, dbatch=3, ubatch=1)
    assert (pl["doppler_batch"], pl["unit_batch"], pl["unit_groups"]) == (3, 1, 1), pl
