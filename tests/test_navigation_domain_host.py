"""The cases of tests/test_navigation_domain_gpu.py with the host twin alone (gat_nav_decode_host): the same case functions, their
`both` replaced by the twin as tests/test_navigation_host.py does for the first grid, so that every input and every expected value
of the device tests is proven here, against the numpy restatement, against what was sent and against the two oracles, before a
device sees it.  Then the oracles themselves: the exhaustive one meets streams with several best paths (at least 10 of its 80
(stream, phase) pairs, and at least 10 of the 30 with seven steps or more, where equal metrics are no artefact of the unknown
register: the decoder's tie rules are on trial), and both refuse a path that is not the decoder's."""
import numpy as np
import pytest

from tests import nav_cases as nc
from tests import nav_ref as ref
from tests import test_navigation_domain_gpu as dom


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture()
def env(g, monkeypatch):
    """the device tests' cases with the twin alone: `both` returns the twin's buffer"""
    from gpuacceleratedtracking_amd import _lib

    def twin(env, fmt, sym, mon, max_frames, min_frames=1, want=nc.OUTPUTS, what=""):
        rc, buf, at = nc.host_call(g, sym, mon, nc.config(_lib, fmt, sym.shape[1], max_frames, min_frames), want)
        assert rc == 0 and nc.canaries_intact(buf, at, want), what
        return buf, at

    monkeypatch.setattr(dom, "both", twin)
    return g, _lib, None, None


@pytest.mark.parametrize("fmt", dom.FORMATS)
def test_twin_many_frames_and_the_rollover(env, fmt):
    dom.test_many_frames_and_the_rollover(env, fmt)


@pytest.mark.parametrize("fmt", dom.FORMATS)
def test_twin_frames_beyond_one_workgroup(env, fmt):
    dom.test_frames_beyond_one_workgroup(env, fmt)


def test_twin_4096_channels(env):
    dom.test_4096_channels_cnav(env)
    dom.test_4096_channels_lnav(env)


@pytest.mark.parametrize("fmt", dom.FORMATS)
def test_twin_capacity_two_to_the_twenty(env, fmt):
    dom.test_capacity_two_to_the_twenty(env, fmt)


@pytest.mark.parametrize("fmt", dom.FORMATS)
def test_twin_counts_outside_the_row(env, fmt):
    dom.test_counts_outside_the_row(env, fmt)


def test_twin_quantiser_edges(env):
    dom.test_quantiser_exact_ties(env)
    dom.test_quantiser_scales(env)


@pytest.mark.parametrize("fmt", dom.FORMATS)
def test_twin_ties_and_seconds_of_the_choice(env, fmt):
    dom.test_ties_and_seconds_of_the_choice(env, fmt)


def test_twin_every_path_of_short_streams(env):
    several, long_ones = dom.every_path_of_short_streams(env)
    print("(stream, phase) pairs with several best input sequences:", several, "of them with seven steps or more:", long_ones)
    assert several >= 10 and long_ones >= 10


def test_twin_calls_in_flight(g):
    """the inputs of the device's unsynchronised calls, and what their frames must hold"""
    from gpuacceleratedtracking_amd import _lib
    dom.in_flight_twin(g, _lib, dom.in_flight_calls())


# ---- the oracles themselves ----------------------------------------------------------------------------------------------------------
def test_the_encoder_from_any_register():
    """fec_encode(bits, state): the tail of a code word is the code of the tail's bits from the register the head left"""
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, 60).astype(np.uint8)
    whole = ref.fec_encode(bits)
    for cut in (1, 5, 6, 7, 33):
        state = 0
        for u in bits[:cut]:
            state = (int(u) << 5) | (state >> 1)
        assert np.array_equal(ref.fec_encode(bits[cut:], state), whole[2 * cut:])
    assert ref.fec_encode(np.ones(4, np.uint8), 63).tolist() == [1] * 8  # five taps each: the inverted stream is a code word
    assert ref.fec_encode(bits[None, :], np.arange(64)).shape == (64, 120)


def test_the_oracles_refuse_a_wrong_path():
    """a clean code word: its own bits pass both oracles with the metric sum |q|, a metric off by one fails; at ten steps the
    best input is the only one and any single wrong bit fails both"""
    rng = np.random.default_rng(2)
    for T in (1, 6, 7, 10):
        bits = rng.integers(0, 2, T).astype(np.uint8)
        q = (16 * (1 - 2 * ref.fec_encode(bits, int(rng.integers(0, 64))).astype(np.int64)))
        metric = int(np.abs(q).sum())
        several = ref.check_exhaustive_ml(q, bits, metric)
        assert ref.path_certificate(q, bits) == metric
        with pytest.raises(AssertionError):
            ref.check_exhaustive_ml(q, bits, metric - 1)
        if T < 10:  # a short stream's first bits trade against the unknown register: several inputs give the same symbols
            continue
        assert several == 1
        for t in range(T):
            wrong = bits.copy()
            wrong[t] ^= 1
            assert ref.path_certificate(q, wrong) < metric
            with pytest.raises(AssertionError):
                ref.check_exhaustive_ml(q, wrong, metric)
    # and at a length beyond brute force
    bits = rng.integers(0, 2, 5000).astype(np.uint8)
    q = 16 * (1 - 2 * ref.fec_encode(bits, 37).astype(np.int64))
    assert ref.path_certificate(q, bits) == 16 * 10000
    bits[2500] ^= 1
    assert ref.path_certificate(q, bits) == 16 * 10000 - 2 * 16 * 10  # the free distance of the code: ten symbols differ


def test_the_oracles_agree_with_the_restatement():
    """the restatement's decoder on the 40 short streams: a best path by enumeration, and the certificate at a long length"""
    for x in dom.ml_streams():
        q = ref.quantise(x, len(x))
        for ph in (0, 1):
            T = (len(x) - ph) // 2
            bits, metric = ref.viterbi(q[None, ph:ph + 2 * T])
            ref.check_exhaustive_ml(q[ph:ph + 2 * T], bits[0], metric[0])
            assert ref.path_certificate(q[ph:ph + 2 * T], bits[0]) == metric[0]
    q = ref.quantise(np.random.default_rng(3).standard_normal(4000), 4000)
    bits, metric = ref.viterbi(q[None, :])
    assert ref.path_certificate(q, bits[0]) == metric[0]
