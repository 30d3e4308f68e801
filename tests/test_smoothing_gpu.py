"""gat_smooth_observables on the device against its host twin, byte for byte on every output, at the shapes where kernels that cut
the epochs into chunks and scan them can go wrong: one epoch, two, a chunk less one, exactly a chunk, one more, three chunks and
seven; one channel, five, sixty-four; windows of 1, 2, 7, a chunk, a chunk and three, every epoch and the largest; arc starts on the
first and the last epoch of a chunk; look-backs across one and several chunk boundaries; a channel with nothing measured; every subset
of the optional outputs; sums that pass 2^64; the same call twice; and the device call refused as the twin is.  The twin itself is
compared with the independent restatement in tests/test_smoothing_host.py."""
import itertools

import numpy as np
import pytest

from tests import smooth_cases as sc

pytestmark = pytest.mark.gpu

OPTIONAL = ("count", "cmc_s", "status", "channels")
CHUNK = 256
EPOCHS = (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 7)
MEASURED, GAP, CMC, RATE = 1, 2, 4, 8


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    assert g.smoothing_plan(1000, 5)["chunk_epochs"] == CHUNK
    return g


def same_bits(dev, host, outputs=OPTIONAL, what=""):
    for name in ("tx_frac_out",) + tuple(outputs):
        a, b = getattr(dev, name), getattr(host, name)
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        assert a.tobytes() == b.tobytes(), (what, name, np.argwhere(a.view(np.uint8).reshape(a.shape + (-1,)) != b.view(np.uint8).reshape(b.shape + (-1,)))[:5])


def edge_case(E: int, K: int, window: int = 7):
    """arc starts on the first and the last epoch of every chunk (slips on channel 0, gaps before them on the last channel), a lock
    mask, gaps, a week wrap, the rate test; the middle channel of five and more without a slip, so that its look-back is the window's"""
    edges = np.array([e for c in range(1, 4) for e in (c * CHUNK - 1, c * CHUNK) if 0 < e < E], dtype=np.int64)
    slips = [(int(e), 0, 400) for e in edges]
    case = sc.synthetic(1000 * E + K, E, K, window=window, slips=slips, mask_p=0.01 if K > 1 else 0.0, week_wrap=True, rate_gate_cycles=0.5,
                        dead_channel=3 if K >= 5 else None)
    if K >= 5:
        gaps = np.random.default_rng(E + K).random((E, K)) < 0.01
        gaps[:, 2] = gaps[:, K - 1] = False
        case.tx_ms[gaps] = -1
        case.valid[:, 2] = 1  # measured throughout
        case.valid[edges, K - 1] = 1
        for e in edges:
            case.valid[e - 1, K - 1] = 0
    return case


@pytest.mark.parametrize("E,K", list(itertools.product(EPOCHS, (1, 5, 64))))
def test_device_equals_twin_over_shapes_and_windows(g, E, K):
    plan = g.smoothing_plan(E, K)
    assert plan["num_chunks"] == -(-E // CHUNK) and plan["lanes"] >= K and plan["rows"] * plan["run_epochs"] == CHUNK
    case = edge_case(E, K)
    dev_obs, host_obs = case.observables(g, "cuda"), case.observables(g)
    kw_dev, kw_host = case.call_kwargs("cuda"), case.call_kwargs()
    for W in sorted({1, 2, 7, CHUNK, CHUNK + 3, E, 65536}):
        kw_dev["window"] = kw_host["window"] = W
        dev = g.smooth_observables(dev_obs, **kw_dev)
        assert dev._host is None  # nothing read back by the call
        host = g.smooth_observables_host(host_obs, **kw_host)
        same_bits(dev, host, what=f"W {W}")
    if E > CHUNK:  # the arcs begin where the case put them
        assert (host.status[CHUNK - 1, 0] & CMC) and (host.status[CHUNK, 0] & CMC)
    if E > 3 * CHUNK and K >= 5:  # a look-back across three chunk boundaries, a channel with nothing measured
        assert host.count[:, 2].max() == E and (host.status[:, 3] == 0).all() and tuple(host.channels[3]) == (0, 0, 0, 0)
        assert host.status[CHUNK, K - 1] & GAP


def test_every_subset_of_the_optional_outputs_and_the_same_call_twice(g):
    case = edge_case(CHUNK + 9, 5, window=CHUNK + 3)
    dev_obs, host = case.observables(g, "cuda"), g.smooth_observables_host(case.observables(g), **case.call_kwargs())
    kw = case.call_kwargs("cuda")
    for r in range(len(OPTIONAL) + 1):
        for subset in itertools.combinations(OPTIONAL, r):
            dev = g.smooth_observables(dev_obs, outputs=subset, **kw)
            same_bits(dev, host, subset, what=str(subset))
            assert set(dev._raw) == {"tx_frac_out", *subset}
    again = g.smooth_observables(dev_obs, **kw)
    same_bits(again, host, what="second call")
    # without the rate test no Doppler is read, without a mask no mask
    kw.update(rate_gate_cycles=None, valid=None)
    plain = case.copy(rate_gate_cycles=None, valid=None)
    same_bits(g.smooth_observables(dev_obs, **kw), g.smooth_observables_host(plain.observables(g), **plain.call_kwargs()), what="no rate test")


def test_sums_passing_two_to_the_64(g):
    case = sc.wrap_case()
    dev = g.smooth_observables(case.observables(g, "cuda"), **case.call_kwargs("cuda"))
    host = g.smooth_observables_host(case.observables(g), **case.call_kwargs())
    same_bits(dev, host)
    n = np.minimum(np.arange(case.E) + 1, case.window)
    want = np.array([0.0 - (float(-(2 ** 30) * int(v) * (int(v) - 1) // 2) * 2.0 ** -48) / float(v) for v in n])
    assert np.array_equal(dev.count[:, 0], n) and dev.tx_frac_out[:, 0].tobytes() == want.tobytes()


@pytest.mark.parametrize("change,code", [(dict(window=0), 2), (dict(window=65537), 2), (dict(cmc_gate_m=0.0), 2), (dict(cmc_gate_m=1200.0), 2),
                                         (dict(rate_gate_cycles=0.0), 2), (dict(carrier_hz=0.0), 1), (dict(epoch_seconds=float("nan")), 1),
                                         (dict(if_hz=float("inf")), 1), (dict(flags=2), 1), (dict(flags=1, rate_gate_cycles=None, no_doppler=True), 1)])
def test_device_call_is_refused_as_the_twin_is(g, change, code):
    import torch

    case = sc.synthetic(5, 20, 3, window=5)
    change = dict(change)
    if change.pop("no_doppler", False):
        case.doppler_hz = None
    kw_dev, kw_host = dict(case.call_kwargs("cuda"), **change), dict(case.call_kwargs(), **change)
    with pytest.raises(g.GatError) as host_err:
        g.smooth_observables_host(case.observables(g), **kw_host)
    torch.cuda.synchronize()
    with pytest.raises(g.GatError) as dev_err:
        g.smooth_observables(case.observables(g, "cuda"), **kw_dev)
    assert host_err.value.status == dev_err.value.status == code
