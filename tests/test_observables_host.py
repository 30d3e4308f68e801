"""gat_observables_host, the host twin of the observables (include/gat.h, "observables"), against the numpy restatement of
tests/obs_ref.py on the histories of tests/obs_cases.py: every integer exactly, the four quotients bit for bit; every status bit
alone with the neighbours' bytes unchanged; every refusal with nothing written; the week's wraps; CNAV with symbol phase 1; the
fraction at the top of a period; both reception modes, the carry of the fraction and a cold start without a measurement; every
subset of the outputs.  No device."""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import obs_cases as oc
from tests import obs_ref as ref


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


INT_OUTPUTS = ("tx_ms", "rx_ms", "carrier_cycles")
FLOAT_OUTPUTS = ("tx_frac", "rx_frac", "carrier_frac", "doppler_hz", "code_rate_hz")


def twin(g, h, mon, nav, frames, outputs=None, **kw):
    cfg = oc.base_config(**kw)
    return g.observables_host(h.records, mon, (nav, frames), outputs=outputs, **cfg)


def restated(h, mon, nav, frames, **kw):
    cfg = oc.base_config(**kw)
    cfg.setdefault("max_frames", frames.shape[1])
    return ref.reference(h.records, mon, nav, frames, **cfg)


def assert_equal(obs, want):
    for name in INT_OUTPUTS:
        assert np.array_equal(obs.host(name), want[name]), name
    for name in FLOAT_OUTPUTS:
        assert obs.host(name).tobytes() == np.ascontiguousarray(want[name], np.float64).tobytes(), name
    ch = obs.channels
    for k, rec in enumerate(want["channels"]):
        for field, value in rec.items():
            got = ch[field][k]
            assert (got.tobytes() == np.float64(value).tobytes()) if field == "edge_fraction" else got == value, (k, field, got, value)


@pytest.fixture(scope="module")
def case():
    return oc.standard()


def test_case_has_wraps_of_0_1_2_and_both_signs(case):
    h = case[0]
    r = h.records
    T = oc.N / oc.FS
    w = np.rint(((r["code_phase_chips"][:-1] + r["code_freq_hz"][:-1] * T) - r["code_phase_chips"][1:]) / oc.LC)
    assert set(np.unique(w)) == {0.0, 1.0, 2.0}
    assert (r["carrier_freq_hz"] > 0).any() and (r["carrier_freq_hz"] < 0).any()
    x = r["code_phase_chips"][case[4], np.arange(h.K)] / oc.LC
    assert ((x < 0.35) | (x > 0.65)).all()


@pytest.mark.parametrize("epochs", [dict(), dict(epoch_first=0, epoch_stride=20), dict(epoch_first=37, epoch_stride=7, num_epochs=11),
                                    dict(epoch_first=700, num_epochs=1), dict(epoch_first=0, num_epochs=1)])
@pytest.mark.parametrize("rx", ["from_tx", (604799990, 0.000987)])
def test_twin_equals_restatement(g, case, epochs, rx):
    h, mon, nav, frames, gk = case
    obs = twin(g, h, mon, nav, frames, rx=rx, **epochs)
    want = restated(h, mon, nav, frames, rx=rx, **epochs)
    assert_equal(obs, want)
    assert (obs.status == 0).all() and (obs.frame_block == gk).all() and (obs.host("tx_ms") >= 0).all()
    # the truth the history was built from
    E = obs.host("tx_ms").shape[0]
    b = epochs.get("epoch_first", 0) + epochs.get("epoch_stride", 1) * np.arange(E)
    assert np.array_equal(obs.host("tx_ms"), h.ms[b]) and obs.host("tx_frac").tobytes() == np.ascontiguousarray(h.tx_frac[b]).tobytes()


def flawed(case, kind):
    """a copy of the case with channel 1 flawed; returns (case, the status channel 1 must show, config)"""
    h, mon, nav, frames, gk = case
    h = oc.History(h.records.copy(), h.ms.copy())
    mon, nav, frames, cfg = mon.copy(), nav.copy(), frames.copy(), {}
    R = ref
    if kind == "nan":
        h.records["carrier_freq_hz"][333, 1] = np.nan
        want = R.BAD_RECORD
    elif kind == "inf_last":
        h.records["code_freq_hz"][h.B, 1] = np.inf
        want = R.BAD_RECORD
    elif kind == "quotient":
        h.records["code_phase_chips"][250, 1] += 0.01
        want = R.BAD_RECORD
    elif kind == "cycles":
        h.records["carrier_phase_cycles"][400, 1] += 0.25
        want = R.BAD_RECORD
    elif kind == "tau_at_epoch":  # a whole period too many: the wraps stay whole, the phase is outside
        h.records["code_phase_chips"][100, 1] += oc.LC
        want = R.BAD_RECORD
    elif kind == "no_bit_sync":
        mon["start"][1] = -1
        want = R.NO_BIT_SYNC
    elif kind == "no_frame_sync":
        nav["frame_offset"][1] = -1
        want = R.NO_FRAME_SYNC
    elif kind == "frame_outside":
        nav["frame_offset"][1] = 36
        want = R.FRAME_OUTSIDE
    elif kind == "no_good_frame":
        frames["status"][1, :] = 0x7FE
        want = R.NO_TOW
    elif kind == "tow_steps":
        nav["tow_steps"][1], cfg["min_tow_steps"] = 1, 2
        nav["tow_steps"][[0, 2, 3]] = 2
        want = R.NO_TOW
    else:
        raise KeyError(kind)
    return (h, mon, nav, frames, gk), want, cfg


@pytest.mark.parametrize("kind", ["nan", "inf_last", "quotient", "cycles", "tau_at_epoch", "no_bit_sync", "no_frame_sync", "frame_outside",
                                  "no_good_frame", "tow_steps"])
def test_every_status_bit_alone(g, case, kind):
    bad, want_status, cfg = flawed(case, kind)
    cfg.update(epoch_first=0, epoch_stride=50, rx=(1000, 0.0))
    if kind == "tow_steps":
        case = (case[0], case[1], bad[2], case[3], case[4])
    good = twin(g, *case[:4], **cfg)
    obs = twin(g, *bad[:4], **cfg)
    assert_equal(obs, restated(*bad[:4], **cfg))
    assert obs.status[1] == want_status and (obs.status[[0, 2, 3]] == 0).all()
    assert (obs.host("tx_ms")[:, 1] == -1).all() and (obs.host("tx_frac")[:, 1] == 0).all()
    others = [0, 2, 3]
    for name in ("tx_ms", "tx_frac", "carrier_cycles", "carrier_frac", "doppler_hz", "code_rate_hz"):
        assert obs.host(name)[:, others].tobytes() == good.host(name)[:, others].tobytes(), name
        if want_status == ref.BAD_RECORD and not name.startswith("tx"):
            assert (obs.host(name)[:, 1] == 0).all(), name
        elif not name.startswith("tx"):
            assert obs.host(name)[:, 1].tobytes() == good.host(name)[:, 1].tobytes(), name
    assert obs.channels[others].tobytes() == good.channels[others].tobytes()
    assert obs.host("rx_ms").tobytes() == good.host("rx_ms").tobytes()


def test_edge_ambiguity_keeps_the_measurement(g):
    case = oc.standard(tau_g_fraction=[0.1, 0.45, 0.58, 0.9])
    obs = twin(g, *case[:4], epoch_stride=100)
    assert_equal(obs, restated(*case[:4], epoch_stride=100))
    assert list(obs.status) == [0, ref.EDGE_AMBIGUOUS, ref.EDGE_AMBIGUOUS, 0] and (obs.host("tx_ms") >= 0).all() and obs.measured.all()
    wide = twin(g, *case[:4], epoch_stride=100, edge_margin=0.5)
    assert (wide.status == ref.EDGE_AMBIGUOUS).all()
    none = twin(g, *case[:4], epoch_stride=100, edge_margin=0.0)
    assert (none.status == 0).all()


@pytest.mark.parametrize("name,week_ms0", [("previous_week", 604794000 - 150), ("tow_0", 604788000 - 150), ("mid", 300000000)])
def test_week_wraps(g, name, week_ms0):
    """frame 0 in the last 6 s of the week (its TOW count is 0), frame 0 just before them (TOW 100799, frame 1's is 0), and in
    every case epochs before the frame: n_b - p* is negative there"""
    case = oc.standard(week_ms0=week_ms0, frame_lead=300)
    h, mon, nav, frames, gk = case
    obs = twin(g, h, mon, nav, frames, epoch_stride=25)
    assert_equal(obs, restated(h, mon, nav, frames, epoch_stride=25))
    b = 25 * np.arange(obs.host("tx_ms").shape[0])
    assert np.array_equal(obs.host("tx_ms"), h.ms[b])
    if name == "previous_week":
        assert (frames["tow"][:, 0] == 0).all() and (obs.frame0_ms == 604794000).all()
        assert (obs.host("tx_ms")[0] > 604790000).all() and (obs.host("tx_ms")[-1] > 604790000).all()
    if name == "tow_0":
        assert (frames["tow"][:, 0] == 100799).all() and (frames["tow"][:, 1] == 0).all()
    assert (b[:, None] < gk[None, :]).any()


def test_transmissions_cross_the_week(g):
    """the frame begins at the first millisecond of the week: the epochs before it lie in the week before"""
    case = oc.standard(week_ms0=604800000 - 150, frame_lead=300)
    h, mon, nav, frames, gk = case
    obs = twin(g, h, mon, nav, frames, epoch_stride=10)
    assert_equal(obs, restated(h, mon, nav, frames, epoch_stride=10))
    tx = obs.host("tx_ms")
    assert (obs.frame0_ms == 0).all() and (frames["tow"][:, 0] == 1).all()
    assert (tx[0] > 604799000).all() and (tx[-1] < 1000).all() and np.array_equal(tx, h.ms[::10])


def test_cnav_symbol_phase_1(g):
    kw = dict(format=1, symbol_blocks=10)
    case = oc.standard(frame_lead=130, K=2, sync=dict(P=2, Pd=10, full=0x3))
    h, mon, nav, frames, gk = case
    assert list(nav["symbol_phase"]) == [1, 1] and list(gk) == [130, 133] and list(mon["start"]) == [0, 3]
    obs = twin(g, h, mon, nav, frames, epoch_stride=64, **kw)
    assert_equal(obs, restated(h, mon, nav, frames, epoch_stride=64, **kw))
    assert (obs.status == 0).all() and np.array_equal(obs.host("tx_ms"), h.ms[::64])
    # read as LNAV the same records name another block and no good frame
    other = twin(g, h, mon, nav, frames, epoch_stride=64)
    assert (other.status & ref.NO_TOW).all()


def test_fraction_at_the_top_of_a_period(g):
    top = float(np.nextafter(float(oc.LC), 0.0))
    h = oc.history(40, [20], [[5990, 5990]], [[top, 0.0]])
    mon, nav, frames, gk = oc.sync_records(h, [6000, 6000], num_frames=1, max_frames=1)
    obs = twin(g, h, mon, nav, frames, epoch_first=20, num_epochs=1)
    assert_equal(obs, restated(h, mon, nav, frames, epoch_first=20, num_epochs=1))
    f = obs.host("tx_frac")[0]
    assert f[0] < 1e-3 and f[0] == min(top / oc.FC, float(np.nextafter(1e-3, 0.0))) and f[1] == 0.0
    assert list(obs.host("tx_ms")[0]) == [5990, 5990] and (obs.status == 0).all() and list(gk) == [29, 30]


def test_reception_carry_and_cold_start(g):
    """2000 samples a block at 2.046 MHz: S * 1000 leaves a remainder, and the fraction carries into the milliseconds"""
    kw = dict(block_samples=2000, block_seconds=2000 / oc.FS)
    case = oc.standard(B=300, frame_lead=60, **kw)
    for rx in ((604799999, 0.00099), "from_tx"):
        obs = twin(g, *case[:4], rx=rx, epoch_stride=3, **kw)
        want = restated(*case[:4], rx=rx, epoch_stride=3, **kw)
        assert_equal(obs, want)
        ms, frac = obs.host("rx_ms").astype(np.int64), obs.host("rx_frac")
        assert (frac >= 0).all() and (frac < 1e-3).all() and (np.diff(frac) < 0).any()
        t = (ms - ms[0]) % 604800000 * 1e-3 + (frac - frac[0])
        assert np.abs(t - 3 * np.arange(len(t)) * 2000 / oc.FS).max() < 1e-12
    assert obs.host("rx_ms")[0] == (obs.host("tx_ms")[0].max() + 68) % 604800000
    # nobody measured: no reception either
    h, mon, nav, frames, gk = case
    mon = mon.copy()
    mon["start"][:] = -1
    cold = twin(g, h, mon, nav, frames, epoch_stride=3, **kw)
    assert_equal(cold, restated(h, mon, nav, frames, epoch_stride=3, **kw))
    assert (cold.host("rx_ms") == -1).all() and (cold.host("rx_frac") == 0).all() and (cold.host("tx_ms") == -1).all()


def test_anchor_is_the_latest_transmission(g, case):
    h, mon, nav, frames, gk = case
    obs = twin(g, h, mon, nav, frames, epoch_first=5, epoch_stride=100)
    tx_ms, tx_frac = obs.host("tx_ms")[0].astype(np.int64), obs.host("tx_frac")[0]
    k = max(range(h.K), key=lambda i: (tx_ms[i], tx_frac[i], -i))
    assert obs.host("rx_ms")[0] == tx_ms[k] + 68 and obs.host("rx_frac")[0] == tx_frac[k]
    assert obs.host("rx_ms")[1] == tx_ms[k] + 168


def test_every_subset_of_the_outputs(g):
    case = oc.standard(B=90, K=3, frame_lead=30)
    full = twin(g, *case[:4], epoch_stride=9)
    from gpuacceleratedtracking_amd.observables import OUTPUTS

    for r in range(1, len(OUTPUTS) + 1):
        for subset in itertools.combinations(OUTPUTS, r):
            obs = twin(g, *case[:4], epoch_stride=9, outputs=subset)
            assert set(obs._raw) == set(subset)
            for name in subset:
                assert obs.host(name).tobytes() == full.host(name).tobytes(), (subset, name)


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def raw_call(g, h, mon, nav, frames, E, cfg, outs, B=None, K=None, nulls=()):
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.observables import OUTPUTS

    ptr = lambda name, a: None if name in nulls else a.ctypes.data  # noqa: E731
    return _lib.load().gat_observables_host(ptr("history", h.records), ptr("mon", mon), ptr("nav", nav), ptr("frames", frames),
                                            h.B if B is None else B, h.K if K is None else K, E, None if "config" in nulls else C.byref(cfg),
                                            *[None if outs.get(n) is None else outs[n].ctypes.data for n in OUTPUTS])


REFUSALS = [
    ("null history", dict(nulls=("history",)), 1), ("null mon", dict(nulls=("mon",)), 1), ("null nav", dict(nulls=("nav",)), 1),
    ("null frames", dict(nulls=("frames",)), 1), ("null config", dict(nulls=("config",)), 1), ("struct_size", dict(cfg=dict(struct_size=92)), 1),
    ("format", dict(cfg=dict(format=2)), 1), ("rx_mode", dict(cfg=dict(rx_mode=2)), 1), ("B", dict(B=0), 1), ("K", dict(K=0), 1), ("E", dict(E=0), 1),
    ("Pd", dict(cfg=dict(symbol_blocks=0)), 1), ("stride", dict(cfg=dict(epoch_stride=0)), 1), ("max_frames", dict(cfg=dict(max_frames=0)), 1),
    ("first", dict(cfg=dict(epoch_first=-1)), 1), ("beyond", dict(cfg=dict(epoch_first=1)), 1), ("beyond by stride", dict(cfg=dict(epoch_stride=2), E=47), 1), ("margin", dict(cfg=dict(edge_margin=0.51)), 1),
    ("margin nan", dict(cfg=dict(edge_margin=float("nan"))), 1), ("margin negative", dict(cfg=dict(edge_margin=-0.01)), 1),
    ("T", dict(cfg=dict(block_seconds=0.0)), 1), ("N", dict(cfg=dict(block_samples=0)), 1), ("no output", dict(no_outputs=True), 1),
    ("travel", dict(cfg=dict(travel_ms=1001)), 2), ("travel negative", dict(cfg=dict(travel_ms=-1)), 2),
    ("rx0_ms", dict(cfg=dict(rx_mode=0, rx0_ms=604800000)), 2), ("rx0_ms negative", dict(cfg=dict(rx_mode=0, rx0_ms=-1)), 2),
    ("rx0_frac", dict(cfg=dict(rx_mode=0, rx0_frac=1e-3)), 2), ("rx0_frac negative", dict(cfg=dict(rx_mode=0, rx0_frac=-1e-9)), 2),
    ("K range", dict(K=4097), 2), ("B range", dict(B=(1 << 20) + 1), 2), ("period", dict(cfg=dict(code_freq_nominal_hz=1.0230001e6)), 2),
    ("code_length", dict(cfg=dict(code_length=0, code_freq_nominal_hz=0.0)), 2), ("fs fraction", dict(cfg=dict(sampling_freq_hz=2.046e6 + 0.5)), 2),
    ("fs large", dict(cfg=dict(sampling_freq_hz=2.0 ** 41)), 2), ("fs zero", dict(cfg=dict(sampling_freq_hz=0.0)), 2),
    ("if_hz", dict(cfg=dict(if_hz=float("inf"))), 2),
]


@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(g, name, change, code):
    from gpuacceleratedtracking_amd.observables import OUTPUTS, obs_config

    h, mon, nav, frames, gk = oc.standard(B=90, K=3, frame_lead=30)
    cfg = obs_config(max_frames=frames.shape[1], **oc.base_config())
    E = change.get("E", 91)
    outs = {n: np.full(91 * 3 * 32, 0x5A, np.uint8) for n in OUTPUTS}
    if change.get("no_outputs"):
        outs = {}
    assert raw_call(g, h, mon, nav, frames, 91, cfg, outs) == 0 if outs else True
    sentinel = {n: np.full(91 * 3 * 32, 0x5A, np.uint8) for n in outs}
    for field, value in change.get("cfg", {}).items():
        setattr(cfg, field, value)
    rc = raw_call(g, h, mon, nav, frames, E, cfg, sentinel, B=change.get("B"), K=change.get("K"), nulls=change.get("nulls", ()))
    assert rc == code, (name, rc)
    assert all((a == 0x5A).all() for a in sentinel.values())
    if "nulls" not in change and not change.get("no_outputs"):  # the plan refuses the same calls, but for the pointers
        from gpuacceleratedtracking_amd import _lib

        p = _lib.ObsPlan()
        p.struct_size = C.sizeof(_lib.ObsPlan)
        assert _lib.load().gat_observables_plan(change.get("B", h.B), change.get("K", h.K), E, C.byref(cfg), C.byref(p)) == code


def test_scratch_at_the_limits(g):
    """the largest call the other limits admit needs about 600 MB of scratch: the 1 GiB refusal has nothing to refuse today"""
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.observables import obs_config

    cfg = obs_config(max_frames=1, **oc.base_config())
    p = _lib.ObsPlan()
    p.struct_size = C.sizeof(_lib.ObsPlan)
    rc = _lib.load().gat_observables_plan(1 << 20, 4096, 1, C.byref(cfg), C.byref(p))
    print("scratch of 2^20 blocks x 4096 channels:", p.scratch_bytes)
    assert rc == 0 and 0 < p.scratch_bytes <= 1 << 30


def test_plan_reports_the_split(g):
    p = g.observables_plan(65536, 12, **oc.base_config(max_frames=5), epoch_stride=20)
    assert p["chunk_blocks"] == 256 and p["num_chunks"] == 256 and p["lanes"] == 16 and p["rows"] * p["lanes"] == p["threads"] == 256
    assert p["run_blocks"] * p["rows"] == p["chunk_blocks"] and p["chunk_workgroups"] == 256 and p["channel_workgroups"] == 3
    p = g.observables_plan(1000, 300, **oc.base_config(max_frames=5))
    assert p["num_chunks"] == 4 and p["channel_group"] == 256 and p["num_groups"] == 2 and p["chunk_workgroups"] == 8
