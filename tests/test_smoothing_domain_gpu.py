"""gat_smooth_observables on the device over the whole domain of tests/smooth_domain.py, byte for byte against the host twin on every
output and against the independent restatement (tests/smooth_ref.py) on status, count and channels: the lanes splits the shapes of
tests/test_smoothing_gpu.py leave out (lanes 2, 4, 16 and 32, and K one past a power of two), arc starts on the first and the last
epoch of a row's run; 64, 66 and 129 chunks, where a lane of sm_channel_kernel holds one, two and three chunks, the lanes past the
last chunk idle, the reset max-scan and the four counts cross lanes that hold several chunks and a look-back crosses every chunk;
every hostile entry on the device; the two gates met exactly.  A clean channel keeps the bytes it has in the calm run on the
device.  The plan's lanes, rows, run_epochs and num_chunks are asserted for each shape: the test fails if the split it was written
for moves.  The twin against the restatement on every byte is tests/test_smoothing_domain_host.py's."""
import numpy as np
import pytest

from tests import smooth_cases as sc
from tests import smooth_domain as sd

pytestmark = pytest.mark.gpu

OUTPUTS = ("tx_frac_out", "count", "cmc_s", "status", "channels")


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def both(g, case, **over):
    """(device, twin) of one call"""
    kw_dev, kw_host = dict(case.call_kwargs("cuda"), **over), dict(case.call_kwargs(), **over)
    assert kw_host["cmc_gate_m"] / sc.C_LIGHT == case.cmc_gate_s  # the restatement's gate is the call's
    dev = g.smooth_observables(case.observables(g, "cuda"), **kw_dev)
    assert dev._host is None  # nothing read back by the call
    return dev, g.smooth_observables_host(case.observables(g), **kw_host)


def same_bits(dev, host, what):
    for name in OUTPUTS:
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        if a.tobytes() != b.tobytes():
            at = np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))
            raise AssertionError((what, name, "differs at", at[:5].tolist()))


def same_as_restatement(dev, ref, what):
    differ = sc.same_bytes({n: getattr(dev, n) for n in ("status", "count", "channels")}, ref)
    assert not differ, (what, differ)


def plan_is(g, E, K):
    plan = g.smoothing_plan(E, K)
    want = sd.expected_plan(E, K)
    assert {n: plan[n] for n in want} == want, (plan, want)
    return plan


@pytest.mark.parametrize("K", sd.LANES_K)
def test_device_equals_twin_on_every_lanes_split(g, K):
    case = sd.lanes_case(K)
    plan = plan_is(g, case.E, K)
    assert plan["lanes"] == {2: 2, 3: 4, 4: 4, 8: 8, 9: 16, 16: 16, 17: 32, 32: 32, 33: 64, 63: 64}[K] and plan["num_chunks"] == 3
    for W in (7, sd.CHUNK + 3):
        dev, host = both(g, case, window=W)
        same_bits(dev, host, (K, W))
        same_as_restatement(dev, sd.reference(case, window=W), (K, W))
    st = dev.status
    assert all(st[e, 0] & sd.CMC for e in case.chunk_edges + case.run_edges) and (st[256, K - 1] & sd.GAP) and (st[512, K - 1] & sd.CMC)


@pytest.mark.parametrize("chunks", sd.DEEP_CHUNKS)
def test_device_equals_twin_with_several_chunks_a_lane(g, chunks):
    case = sd.deep_case(chunks)
    plan = plan_is(g, case.E, case.K)
    assert plan["num_chunks"] == chunks and -(-plan["num_chunks"] // 64) == {64: 1, 66: 2, 129: 3}[chunks] and plan["lanes"] == 8
    for W in sd.DEEP_WINDOWS:
        dev, host = both(g, case, window=W)
        same_bits(dev, host, (chunks, W))
        same_as_restatement(dev, sd.reference(case, window=W), (chunks, W))
        assert dev.count[:, 0].max() == min(case.E, W) == dev.count[case.E - 1, 0]  # a look-back over every chunk at the largest window
    assert tuple(dev.channels[1]) == (sd.CHUNK, 1, 0, 0) and tuple(dev.channels[2]) == (1, 1, 0, 0) and tuple(dev.channels[3]) == (0, 0, 0, 0)
    assert dev.status[case.E - 1, 2] == sd.M | sd.GAP and dev.channels["cmc_resets"][4] >= chunks - 1


def test_device_equals_twin_on_every_hostile_entry(g):
    base = sd.hostile_base()
    plan = plan_is(g, base.E, base.K)
    assert plan["lanes"] == 8 and plan["run_epochs"] == 8 and sd.AT[2] % 8 == 3
    calm, calm_host = both(g, base)
    same_bits(calm, calm_host, "calm")
    labels = set()
    for t in sd.hostile_tiles():
        what = [en.label for en, _ in t.entries]
        dev, host = both(g, t.case)
        same_bits(dev, host, what)
        same_as_restatement(dev, sd.reference(t.case), what)
        for en, k in t.entries:
            labels.add(en.label)
            for e, want in en.want.items():
                assert (dev.status[e, 1:] == want).all() if k is None else dev.status[e, k] == want, (en.label, e)
        for k in t.clean:  # a clean channel keeps its bytes against the calm run on the device
            for name in OUTPUTS[:4]:
                assert getattr(dev, name)[:, k].tobytes() == getattr(calm, name)[:, k].tobytes(), (what, name, k)
            assert dev.channels[k] == calm.channels[k]
    assert len(labels) == 37


def test_the_gates_are_met_exactly_on_the_device(g):
    case = sd.gate_case()
    plan_is(g, case.E, case.K)
    dev, host = both(g, case)
    same_bits(dev, host, "gates")
    same_as_restatement(dev, sd.reference(case), "gates")
    M, CMC, RATE = sd.M, sd.CMC, sd.RATE
    assert dev.status[253:259, 0].tolist() == [M, M, M, M | CMC, M | CMC, M] and dev.status[253:259, 1].tolist() == [M, M, M, M | RATE, M | RATE, M]
    assert dev.cmc_s[254, 0] == -(2.0 ** -18) and dev.cmc_s[255, 0] == 0.0
