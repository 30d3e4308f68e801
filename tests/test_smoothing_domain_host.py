"""The host twin gat_smooth_observables_host over the whole domain gat.h admits (tests/smooth_domain.py), against the independent
restatement (tests/smooth_ref.py) on every byte of every output: every split of a chunk's workgroup into rows and lanes, 64, 66 and
129 chunks (a lane of the channel kernel holds one, two and three of them) at windows 7, 257 and 65536, every hostile entry -- the
int64 extremes of the cycle count, fractions whose difference overflows, values that are not finite, a Doppler pair whose mean
overflows, the edges of tx_ms and rx_ms, dms at +-1000 and +-1001, the half-week wrap edges, lock mask bytes -- and the two gates
met exactly.  The status bits every entry's label names are asserted against the restatement where the cases are built.  A clean
channel keeps the bytes it has without the hostile ones.  The plan's split is asserted for every shape the device test runs.  Needs
no device."""
import numpy as np
import pytest

from tests import smooth_cases as sc
from tests import smooth_domain as sd


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    return g


def twin(case, **over):
    rc, got = sc.host_call(case, cfg=sc.smooth_cfg(**case.config(**over)))
    assert rc == 0
    return got


def check(case, what, **over):
    got = twin(case, **over)
    differ = sc.same_bytes(got, sd.reference(case, **over))
    assert not differ, (what, differ)
    return got


@pytest.mark.parametrize("K", sd.LANES_K)
def test_twin_equals_restatement_on_every_lanes_split(g, K):
    case = sd.lanes_case(K)
    plan = g.smoothing_plan(case.E, K)
    assert {n: plan[n] for n in sd.expected_plan(case.E, K)} == sd.expected_plan(case.E, K)
    got = check(case, K)
    assert got["channels"]["arcs"][0] >= len(case.chunk_edges) + len(case.run_edges) and (got["count"][:, 0] == 7).any()


@pytest.mark.parametrize("chunks", sd.DEEP_CHUNKS)
def test_twin_equals_restatement_over_many_chunks(g, chunks):
    case = sd.deep_case(chunks)
    plan = g.smoothing_plan(case.E, case.K)
    assert {n: plan[n] for n in sd.expected_plan(case.E, 5)} == sd.expected_plan(case.E, 5) and plan["num_chunks"] == chunks
    assert -(-plan["num_chunks"] // 64) == case.per == {64: 1, 66: 2, 129: 3}[chunks]
    for W in sd.DEEP_WINDOWS:
        got = check(case, (chunks, W), window=W)
        assert got["count"][:, 0].max() == min(case.E, W) and got["count"][case.E - 1, 2] == 1 and not got["count"][:, 3].any()


def test_twin_equals_restatement_on_every_hostile_entry_and_disturbs_no_clean_channel():
    calm = twin(sd.hostile_base())
    labels = set()
    for t in sd.hostile_tiles():
        got = check(t.case, [en.label for en, _ in t.entries])
        for en, k in t.entries:
            labels.add(en.label)
            for e, want in en.want.items():  # the label's bits: the restatement's, asserted when the tile was built
                assert (got["status"][e, 1:] == want).all() if k is None else got["status"][e, k] == want, (en.label, e)
        for k in t.clean:
            for name in ("tx_frac_out", "count", "cmc_s", "status"):
                assert got[name][:, k].tobytes() == calm[name][:, k].tobytes(), (name, k)
            assert got["channels"][k] == calm["channels"][k]
        assert np.isfinite(got["cmc_s"]).all() and (got["count"] >= 0).all() and (got["count"] <= 100).all()
    assert len(labels) == 37


def test_the_gates_are_met_exactly():
    case = sd.gate_case()
    got = check(case, "gates")
    M, CMC, RATE = sd.M, sd.CMC, sd.RATE
    assert got["status"][253:259, 0].tolist() == [M, M, M, M | CMC, M | CMC, M]
    assert got["status"][253:259, 1].tolist() == [M, M, M, M | RATE, M | RATE, M]
    assert got["cmc_s"][254, 0] == -(2.0 ** -18) and got["cmc_s"][255, 0] == 0.0  # q = -2^30, then +2^30
    assert tuple(got["channels"][0]) == (case.E, 3, 2, 0) and tuple(got["channels"][1]) == (case.E, 3, 0, 2)
