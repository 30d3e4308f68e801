"""gat_observables on the device against its host twin, byte for byte, over the work split of csrc/gat_obs_plan.h.  With C the
plan's chunk length: B in {1, 2, C - 1, C, C + 1, 2 C + 3}; K in {1, 3, 64, 65, the first K of the second channel group + 1}; epochs
at block 0 only, at record B only, at every block, with a stride above C (whole chunks hold none) and from a first epoch beyond
chunk 0; a frame block in the last chunk; a bad record in the halo position of a chunk; both formats and both reception modes; a
second identical call with identical bytes.  The histories are those of tests/obs_cases.py, whose truth the host tests hold the
twin to."""
import functools

import numpy as np
import pytest

from tests import obs_cases as oc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@functools.lru_cache(maxsize=None)
def plan_constants():
    import gpuacceleratedtracking_amd as g

    p = g.observables_plan(1000, 3, **oc.base_config(max_frames=4))
    q = g.observables_plan(1000, 4096, **oc.base_config(max_frames=4))
    return p["chunk_blocks"], q["channel_group"]


def device(g, case, **cfg):
    import torch

    h, mon, nav, frames, _ = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    hist = t(h.records).reshape(h.B + 1, h.K, 40)
    return g.observables(hist, t(mon), (t(nav), t(frames)), **oc.base_config(**cfg))


def both(g, case, **cfg):
    from gpuacceleratedtracking_amd.observables import OUTPUTS

    h, mon, nav, frames, _ = case
    dev = device(g, case, **cfg)
    assert dev._host is None
    host = g.observables_host(h.records, mon, (nav, frames), **oc.base_config(**cfg))
    for name in OUTPUTS:
        a, b = dev.host(name), host.host(name)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), (name, np.argwhere(np.atleast_1d(a != b))[:5])
    return dev, host


def small_case(B, K, **kw):
    lead = min(max(B // 3, 1), 120) if B > 2 else 1
    return oc.standard(B, K, frame_lead=lead, spread=3 if B >= 64 else 0, **kw)


def sizes():
    C, G = plan_constants()
    return [1, 2, C - 1, C, C + 1, 2 * C + 3], [1, 3, 64, 65, G + 2]


def test_plan_constants():
    C, G = plan_constants()
    assert C == 256 and G == 256  # the sizes below are derived from the plan; this only pins what the docstring's numbers mean


@pytest.mark.parametrize("ki", range(5))
@pytest.mark.parametrize("bi", range(6))
def test_every_block_an_epoch(g, bi, ki):
    Bs, Ks = sizes()
    B, K = Bs[bi], Ks[ki]
    dev, _ = both(g, small_case(B, K))
    assert dev.host("tx_ms").shape == (B + 1, K)
    if B > 2:
        assert (dev.status == 0).all() and (dev.host("tx_ms") >= 0).all()


EPOCHS = {"block_0": dict(epoch_first=0, num_epochs=1), "record_B": dict(epoch_first=515, num_epochs=1), "every_block": dict(),
          "stride_above_chunk": dict(epoch_first=3, epoch_stride=300), "first_beyond_chunk_0": dict(epoch_first=260, epoch_stride=7),
          "stride_chunk": dict(epoch_first=0, epoch_stride=256)}


@pytest.mark.parametrize("rx", ["from_tx", (604799998, 0.00099)])
@pytest.mark.parametrize("name", list(EPOCHS))
def test_epoch_placements(g, name, rx):
    case = small_case(515, 3)
    dev, host = both(g, case, rx=rx, **EPOCHS[name])
    E = dev.host("rx_ms").shape[0]
    b = EPOCHS[name].get("epoch_first", 0) + EPOCHS[name].get("epoch_stride", 1) * np.arange(E)
    assert np.array_equal(dev.host("tx_ms"), case[0].ms[b]) and (dev.host("rx_ms") >= 0).all()


def test_frame_block_in_the_last_chunk(g):
    case = oc.standard(515, 5, frame_lead=513, spread=0)
    assert (case[4] == 513).all()
    dev, _ = both(g, case, epoch_stride=5)
    assert (dev.status == 0).all() and (dev.frame_block == 513).all()
    # ... and at record B itself
    case = oc.standard(512, 5, frame_lead=512, spread=0)
    dev, _ = both(g, case, epoch_stride=64)
    assert (dev.status == 0).all() and (dev.frame_block == 512).all() and np.array_equal(dev.host("tx_ms"), case[0].ms[::64])


@pytest.mark.parametrize("where", [256, 512, 515, 0])
@pytest.mark.parametrize("field", ["code_phase_chips", "carrier_freq_hz"])
def test_bad_record_in_a_halo_position(g, where, field):
    """record 256 is the halo of chunk 0 and the first record of chunk 1, record 515 the last one's halo and nobody's first"""
    h, mon, nav, frames, gk = small_case(515, 4)
    h = oc.History(h.records.copy(), h.ms)
    h.records[field][where, 2] = np.nan
    dev, _ = both(g, (h, mon, nav, frames, gk), epoch_stride=17)
    assert list(dev.status) == [0, 0, 1, 0] and (dev.host("tx_ms")[:, 2] == -1).all() and (dev.host("tx_ms")[:, [0, 1, 3]] >= 0).all()


def test_status_bits_and_a_cold_start_without_measurement(g):
    h, mon, nav, frames, gk = small_case(300, 6)
    mon, nav, frames = mon.copy(), nav.copy(), frames.copy()
    mon["start"][0] = -1
    nav["frame_offset"][1] = -1
    nav["frame_offset"][2] = 40
    frames["status"][3] = 0
    dev, _ = both(g, (h, mon, nav, frames, gk), epoch_stride=10)
    assert list(dev.status) == [2, 4, 8, 16, 0, 0]
    mon["start"][:] = -1
    dev, _ = both(g, (h, mon, nav, frames, gk), epoch_stride=10)
    assert (dev.host("rx_ms") == -1).all() and (dev.host("tx_ms") == -1).all()


def test_cnav(g):
    case = oc.standard(600, 7, frame_lead=130, sync=dict(P=2, Pd=10, full=0x3))
    dev, _ = both(g, case, format=1, symbol_blocks=10, epoch_stride=3)
    assert (dev.status == 0).all() and set(case[2]["symbol_phase"]) == {0, 1}


def test_anchor_over_many_channels(g):
    """more channels than the anchor's wave has lanes, the latest transmission among the last ones"""
    case = small_case(300, 130)
    dev, _ = both(g, case, epoch_first=7, epoch_stride=50)
    tx_ms, tx_frac = dev.host("tx_ms")[0].astype(np.int64), dev.host("tx_frac")[0]
    k = max(range(130), key=lambda i: (tx_ms[i], tx_frac[i], -i))
    assert dev.host("rx_ms")[0] == tx_ms[k] + 68 and dev.host("rx_frac")[0] == tx_frac[k]


def test_subsets_of_the_outputs_and_a_second_call(g):
    from gpuacceleratedtracking_amd.observables import OUTPUTS

    case = small_case(515, 65)
    first, _ = both(g, case, epoch_stride=4)
    second = device(g, case, epoch_stride=4)
    for name in OUTPUTS:
        assert second.host(name).tobytes() == first.host(name).tobytes(), name
    for subset in (("tx_ms",), ("rx_frac",), ("channels",), ("carrier_cycles", "doppler_hz"), ("tx_ms", "tx_frac", "rx_ms", "rx_frac")):
        h, mon, nav, frames, _ = case
        import torch

        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
        obs = g.observables(t(h.records).reshape(h.B + 1, h.K, 40), t(mon), (t(nav), t(frames)), outputs=subset, **oc.base_config(epoch_stride=4))
        assert set(obs._raw) == set(subset)
        for name in subset:
            assert obs.host(name).tobytes() == first.host(name).tobytes(), (subset, name)


def test_refusal_before_any_launch(g):
    import torch

    case = small_case(64, 3)
    h, mon, nav, frames, _ = case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()  # noqa: E731
    with pytest.raises(g.GatError) as e:
        g.observables(t(h.records).reshape(65, 3, 40), t(mon), (t(nav), t(frames)), **oc.base_config(epoch_stride=0))
    assert e.value.status == 1
    with pytest.raises(g.GatError) as e:
        g.observables(t(h.records).reshape(65, 3, 40), t(mon), (t(nav), t(frames)), **oc.base_config(travel_ms=2000))
    assert e.value.status == 2
