"""The carrier smoothing's host twin (gat_smooth_observables_host) against an independent restatement of the rule
(tests/smooth_ref.py: exact Python integers, no modular arithmetic): the same bytes on every output over random cases with gaps, lock
masks, entries that are not finite, week wraps of tx_ms and rx_ms and arcs of every length around W; the sums passing 2^64; the
physics (white code noise of 1 m behind a window of 100 leaves a tenth); a slip, a Doppler entry off and a masked epoch flagged
where they are and nowhere else; every documented refusal with nothing written."""
import ctypes as C
import math

import numpy as np
import pytest

import gpuacceleratedtracking_amd._lib as _lib
from tests import fix_cases as fc
from tests import fix_ref
from tests import smooth_cases as sc

MEASURED, GAP, CMC, RATE = 1, 2, 4, 8
ARG, RANGE = 1, 2  # GAT_ERR_ARG, GAT_ERR_RANGE


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def check(case, outputs=sc.OUTPUTS):
    rc, got = sc.host_call(case, outputs)
    assert rc == 0
    differ = sc.same_bytes(got, case.reference())
    assert not differ, differ
    return got


@pytest.mark.parametrize("seed", range(6))
def test_twin_equals_restatement_on_random_cases(seed):
    rng = np.random.default_rng(100 + seed)
    E, K, W = int(rng.integers(40, 400)), int(rng.integers(1, 9)), int(rng.choice([1, 2, 7, 30, 65536]))
    slips = [(int(rng.integers(1, E)), int(rng.integers(0, K)), int(rng.choice([-300, 120, 100000]))) for _ in range(4)]
    case = sc.synthetic(seed, E, K, window=W, slips=slips, gap_p=0.03 * (seed % 3), mask_p=0.02 * (seed % 2), nonfinite=seed,
                        week_wrap=seed % 2 == 1, rate_gate_cycles=None if seed % 3 == 0 else 0.5)
    got = check(case)
    assert (got["status"] & MEASURED).any() and (got["count"] == min(W, 5)).any()


def test_arcs_of_every_length_around_the_window():
    W = 9
    lengths = [1, 2, W - 1, W, W + 1, 2 * W, 2 * W + 1, 3]
    starts = np.cumsum([5] + lengths)
    case = sc.synthetic(7, int(starts[-1]) + 4 * W, 3, window=W, slips=[(int(s), 1, 500) for s in starts])
    got = check(case)
    assert set(np.flatnonzero(got["status"][:, 1] & CMC)) == set(int(s) for s in starts)
    for s, n in zip(starts, lengths):
        assert list(got["count"][s:s + n, 1]) == [min(i + 1, W) for i in range(n)]
    assert got["channels"]["arcs"][1] == len(starts) + 1 and got["channels"]["cmc_resets"][1] == len(starts)


def test_sums_passing_two_to_the_64_stay_exact():
    case = sc.wrap_case()
    rc, got = sc.host_call(case)
    assert rc == 0
    E, W = case.E, case.window
    n = np.minimum(np.arange(E) + 1, W).astype(np.int64)
    assert 2 ** 30 * (E - 1) * E // 2 > 2 ** 64  # SS at the last epoch
    S = [-(2 ** 30) * int(v) * (int(v) - 1) // 2 for v in n]
    want = np.array([0.0 - (float(s) * 2.0 ** -48) / float(v) for s, v in zip(S, n)])
    assert np.array_equal(got["count"][:, 0], n) and got["tx_frac_out"][:, 0].tobytes() == want.tobytes()
    assert got["cmc_s"][:, 0].tobytes() == (2.0 ** -18 * np.arange(E)).tobytes()
    assert not sc.same_bytes(got, case.reference())


def physics_case(E=600, seed=11):
    """five satellites and the site of fix_cases' ``short`` case, a static receiver, a reception a second; the carrier phase exact (any
    integer ambiguities, an IF of 4.2 kHz), white noise of 1 m on the code"""
    base = fc.case("short", 30, 5, 8)
    rng = np.random.default_rng(seed)
    xyz, bias = fc.ground(*fc.RECEIVERS[0]) + np.array([12.0, -30.0, 7.0]), 1.7e-4
    rx_ms = (244800000 + 600000 + 1000 * np.arange(E)).astype(np.int32)
    rx_frac = np.full(E, 0.000123456)
    rows = [fix_ref.transmit_times(base.ephs, xyz, int(rx_ms[e]), float(rx_frac[e]), bias) for e in range(E)]
    tx_ms, tx_frac = np.stack([r[0] for r in rows]).astype(np.int32), np.stack([r[1] for r in rows])
    assert (np.stack([r[2] for r in rows]) > fc.SIN_5_DEG).all()
    if_hz, Te = 4200.0, 1.0
    P = (rx_ms[:, None].astype(np.int64) - tx_ms).astype(np.longdouble) / 1000 + (rx_frac[:, None].astype(np.longdouble) - tx_frac)
    phase = rng.integers(-10 ** 8, 10 ** 8, 5)[None, :].astype(np.longdouble) + np.longdouble(if_hz * Te) * np.arange(E)[:, None] - np.longdouble(sc.FL) * P
    cycles = np.floor(phase)
    noisy = tx_frac + rng.standard_normal(tx_frac.shape) * 1.0 / sc.C_LIGHT
    case = sc.Case(tx_ms=tx_ms, tx_frac=noisy, rx_ms=rx_ms, rx_frac=rx_frac, carrier_cycles=cycles.astype(np.int64),
                   carrier_frac=(phase - cycles).astype(np.float64), doppler_hz=None, valid=None, window=100, if_hz=if_hz, epoch_seconds=Te,
                   cmc_gate_s=15.0 / sc.C_LIGHT, rate_gate_cycles=None)
    return case, base.ephs, xyz


def test_white_code_noise_behind_the_window_leaves_a_tenth(g):
    """The smoothed pseudorange is L_e + mean over W epochs of (P_j - L_j): the carrier is exact, so its error is the mean of W
    independent code errors, sigma / sqrt(W) = 0.1 sigma for W = 100; the fix is linear in the pseudorange errors at this size, so
    the position error's rms scales alike.  Bound 0.2: a factor 2 for the finite sample (500 epochs behind the fill are five
    independent windows).  Measured: 0.0991."""
    case, ephs, xyz = physics_case()
    rc, got = sc.host_call(case)
    assert rc == 0 and (got["status"][1:] == MEASURED).all() and (got["status"][0] == MEASURED | GAP).all()
    assert (got["count"][case.window:] == case.window).all()
    sent = [g.Ephemeris.from_record(r) for r in ephs]
    raw = g.position_fix_host(sent, case.tx_ms, case.tx_frac, case.rx_ms, case.rx_frac)
    smooth = g.position_fix_host(sent, case.tx_ms, got["tx_frac_out"], case.rx_ms, case.rx_frac)
    assert (raw.status == 0).all() and (smooth.status == 0).all()
    behind = slice(case.window, None)
    rms = lambda f: math.sqrt(np.mean(np.sum((f.xyz[behind] - xyz[None, :]) ** 2, axis=1)))  # noqa: E731
    ratio = rms(smooth) / rms(raw)
    print(f"position error rms: raw {rms(raw):.3f} m, smoothed {rms(smooth):.3f} m, ratio {ratio:.4f} (derived 0.1, bound 0.2)")
    assert ratio <= 0.2
    # the Python layer on an Observables: the same bytes
    via = g.smooth_observables_host(case.observables(g), **case.call_kwargs())
    assert via.tx_frac_out.tobytes() == got["tx_frac_out"].tobytes() and via.status.tobytes() == got["status"].tobytes()
    assert via.channels.tobytes() == got["channels"].tobytes() and (via.measured == case.E).all() and (via.arcs == 1).all()


def test_slip_is_flagged_where_it_is_and_nowhere_else():
    clean = sc.synthetic(21, 120, 4, window=30, gate_m=10.0)
    slipped = sc.synthetic(21, 120, 4, window=30, gate_m=10.0, slips=[(57, 2, 200)])  # 200 cycles = 38 m
    _, a = sc.host_call(clean)
    _, b = sc.host_call(slipped)
    assert (a["status"][1:] == MEASURED).all()
    st = b["status"].copy()
    assert st[57, 2] == MEASURED | CMC
    st[57, 2] = MEASURED
    assert np.array_equal(st, a["status"])
    assert b["count"][57, 2] == 1 and b["count"][56, 2] == 30 and b["count"][58, 2] == 2 and b["cmc_s"][57, 2] == 0.0
    others = [0, 1, 3]
    for name in ("tx_frac_out", "count", "cmc_s", "status"):
        assert a[name][:, others].tobytes() == b[name][:, others].tobytes(), name
    assert a["channels"][others].tobytes() == b["channels"][others].tobytes()
    assert tuple(b["channels"][2]) == (120, 2, 1, 0)
    assert not sc.same_bytes(b, slipped.reference())


def test_doppler_off_sets_rate_and_a_masked_epoch_gives_gap_at_the_next():
    case = sc.synthetic(22, 80, 3, window=20, rate_gate_cycles=0.5)
    _, clean = sc.host_call(case)
    assert (clean["status"][1:] == MEASURED).all()
    case.doppler_hz[40, 1] += 200.0  # 0.5 * 200 Hz * 0.02 s = 2 cycles in the trapezoids of epochs 40 and 41
    case.valid = np.ones((80, 3), np.uint8)
    case.valid[10, 0] = 0
    got = check(case)
    want = clean["status"].copy()
    want[40, 1] = want[41, 1] = MEASURED | RATE
    want[10, 0], want[11, 0] = 0, MEASURED | GAP
    assert np.array_equal(got["status"], want)
    assert got["count"][10, 0] == 0 and got["count"][11, 0] == 1 and got["tx_frac_out"][10, 0] == case.tx_frac[10, 0]
    assert tuple(got["channels"][1]) == (80, 3, 0, 2) and tuple(got["channels"][0]) == (79, 2, 0, 0)


REFUSALS = [
    ("null tx_ms", dict(null="tx_ms"), ARG), ("null tx_frac", dict(null="tx_frac"), ARG), ("null rx_ms", dict(null="rx_ms"), ARG),
    ("null rx_frac", dict(null="rx_frac"), ARG), ("null cycles", dict(null="carrier_cycles"), ARG), ("null frac", dict(null="carrier_frac"), ARG),
    ("null config", dict(no_cfg=True), ARG), ("null tx_frac_out", dict(no_out=True), ARG), ("struct_size", dict(struct_size=48), ARG),
    ("E", dict(E=0), ARG), ("K", dict(K=0), ARG), ("flag", dict(flags=2), ARG), ("reserved", dict(reserved=1), ARG),
    ("rate without doppler", dict(flags=1, rate_gate_cycles=0.5, null="doppler_hz"), ARG),
    ("carrier 0", dict(carrier_hz=0.0), ARG), ("carrier inf", dict(carrier_hz=math.inf), ARG), ("carrier nan", dict(carrier_hz=math.nan), ARG),
    ("epoch 0", dict(epoch_seconds=0.0), ARG), ("epoch -", dict(epoch_seconds=-1.0), ARG), ("epoch inf", dict(epoch_seconds=math.inf), ARG),
    ("if nan", dict(if_hz=math.nan), ARG), ("if inf", dict(if_hz=-math.inf), ARG),
    ("W 0", dict(window=0), RANGE), ("W big", dict(window=65537), RANGE), ("gate 0", dict(cmc_gate_s=0.0), RANGE),
    ("gate big", dict(cmc_gate_s=np.nextafter(2.0 ** -18, 1.0)), RANGE), ("gate nan", dict(cmc_gate_s=math.nan), RANGE),
    ("rate gate 0", dict(flags=1, rate_gate_cycles=0.0), RANGE), ("rate gate inf", dict(flags=1, rate_gate_cycles=math.inf), RANGE),
    ("rate gate nan", dict(flags=1, rate_gate_cycles=math.nan), RANGE), ("K 65", dict(K=65), RANGE), ("E big", dict(E=1048577), RANGE),
    ("scratch", dict(E=1048576, K=64), RANGE),
]


@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal_writes_nothing(name, change, code):
    """GAT_ERR_ARG is 1, GAT_ERR_RANGE 2.  The arrays are those of a small case whatever E and K say: a refused call reads none."""
    case = sc.synthetic(1, 12, 3, window=5)
    change = dict(change)
    a = {n: (None if v is None else np.ascontiguousarray(v)) for n, v in zip(sc.ARRAYS, case.arrays())}
    if "null" in change:
        a[change.pop("null")] = None
    E, K = change.pop("E", case.E), change.pop("K", case.K)
    no_cfg, no_out = change.pop("no_cfg", False), change.pop("no_out", False)
    struct_size = change.pop("struct_size", None)
    cfg = sc.smooth_cfg(**case.config(**change))
    if struct_size is not None:
        cfg.struct_size = struct_size
    out = {n: np.full(case.K * 16 if n == "channels" else case.E * case.K * np.dtype(sc.OUT_DTYPES[n]).itemsize, 0x5A, np.uint8) for n in sc.OUTPUTS}
    before = {n: v.copy() for n, v in out.items()}
    ptr = lambda v: None if v is None else v.ctypes.data  # noqa: E731
    lib = _lib.load()
    rc = lib.gat_smooth_observables_host(*[ptr(a[n]) for n in sc.ARRAYS], E, K, None if no_cfg else C.byref(cfg),
                                         *[None if (no_out and n == "tx_frac_out") else ptr(out[n]) for n in sc.OUTPUTS])
    assert rc == code
    assert all(np.array_equal(out[n], before[n]) for n in out)
    if not any(k in name for k in ("null", "rate without")):  # the plan refuses what does not hang on a pointer alike
        plan = _lib.SmoothPlan()
        plan.struct_size = C.sizeof(_lib.SmoothPlan)
        assert lib.gat_smooth_observables_plan(E, K, C.byref(cfg), C.byref(plan)) == code
        assert plan.num_chunks == 0 and plan.scratch_bytes == 0


def test_plan_reports_the_split(g):
    p = g.smoothing_plan(3 * 256 + 7, 5, window=100)
    assert p["chunk_epochs"] == 256 and p["num_chunks"] == 4 and p["lanes"] == 8 and p["rows"] == 32 and p["run_epochs"] == 8
    assert p["threads"] == 256 and p["chunk_workgroups"] == 4 and p["channel_workgroups"] == 2 and p["output_workgroups"] == (775 * 5 + 255) // 256
    assert p["lds_bytes"] == 256 * 40 and 0 < p["scratch_bytes"] <= 1 << 30
    assert g.smoothing_plan(1048576, 48)["scratch_bytes"] <= 1 << 30
