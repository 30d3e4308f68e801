"""The navigation data layer without a device: the package's surface; the LNAV parity by the masks the library uses against the
parity by the six equations of the specification (tests/nav_ref.py) on random words, with every single-bit error caught; the
CRC-24Q check value; the encoder's impulse response; the package's encoders against the restatement's; the host twin
(gat_nav_decode_host) against the restatement, bit for bit, over the grid of the device tests with canaries around every output;
the Python result; every refusal with every output untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import nav_cases as nc
from tests import nav_ref as ref
from tests import test_navigation_gpu as grid

ARG, RANGE = 1, 2
MASKS = (0xBB1F3480, 0x5D8F9A40, 0xAEC7CD00, 0x5763E680, 0x6BB1F340, 0x8B7A89C0)


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

    monkeypatch.setattr(grid, "both", twin)
    return g, _lib, None, None


def test_the_surface(g):
    """declared, bound and exported (on the parent commit none of it exists)"""
    from gpuacceleratedtracking_amd import _lib
    lib = g.load_library()
    for name in ("gat_nav_decode", "gat_nav_decode_host", "gat_nav_decode_plan"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("decode_navigation", "decode_navigation_host", "nav_plan", "nav_format_for", "lnav_subframe", "cnav_message", "cnav_fec_encode"):
        assert callable(getattr(g, name))
    assert callable(g.TrackingLoop.navigation)
    assert g.nav_format_for(g.GPSL1) == _lib.GAT_NAV_LNAV == 0 and g.nav_format_for("GPSL5") == _lib.GAT_NAV_CNAV == 1
    with pytest.raises(ValueError):
        g.nav_format_for("GALE1")
    p = g.nav_plan(12, 1000, "CNAV")
    assert (p["num_phases"], p["bit_capacity"], p["num_candidates"], p["trellis_workgroups"], p["quantise_workgroups"]) == (2, 500, 1200, 24, 12)
    assert p["slice_workgroups"] == 0 and p["scratch_bytes"] >= 12 * (1000 + 2 * 500 * 8 + 1200 * 4)
    p = g.nav_plan(12, 1000, "LNAV", max_frames=5)
    assert (p["num_phases"], p["bit_capacity"], p["num_candidates"], p["trellis_workgroups"]) == (1, 1000, 600, 0)
    assert p["slice_workgroups"] == 47 and p["score_workgroups"] == 29 and p["pick_workgroups"] == 3 and p["frame_workgroups"] == 1


def mask_parity(word32):
    """the six parity bits as the library computes them: the word with D29* and D30* on top, de-inverted, through the masks"""
    if word32 & 0x40000000:
        word32 ^= 0x3FFFFFC0
    return [bin(word32 & m).count("1") & 1 for m in MASKS]


def test_parity_masks_are_the_equations():
    rng = np.random.default_rng(1)
    for _ in range(2000):
        d, a, b = [int(v) for v in rng.integers(0, 2, 24)], int(rng.integers(0, 2)), int(rng.integers(0, 2))
        sent = ref.lnav_encode_word(d, a, b)
        word = (a << 31) | (b << 30) | ref.value(sent)
        assert mask_parity(word) == sent[24:] == ref.lnav_parity(d, a, b)
        assert ref.lnav_check(sent, a, b) == (True, d)
    # no single-bit error of the thirty sent bits or of the two starred ones passes
    d, a, b = [int(v) for v in rng.integers(0, 2, 24)], 1, 1
    sent = ref.lnav_encode_word(d, a, b)
    for i in range(30):
        bad = list(sent)
        bad[i] ^= 1
        assert not ref.lnav_check(bad, a, b)[0] and mask_parity((a << 31) | (b << 30) | ref.value(bad)) != bad[24:]
    assert not ref.lnav_check(sent, a ^ 1, b)[0] and not ref.lnav_check(sent, a, b ^ 1)[0]


def test_crc24q_check_value(g):
    msg = np.unpackbits(np.frombuffer(b"123456789", np.uint8))
    assert g.crc24q(msg) == ref.crc24q(msg) == 0xCDE703
    body = np.random.default_rng(2).integers(0, 2, 276)
    whole = list(body) + ref.bits_of(ref.crc24q(body), 24)
    assert g.crc24q(whole) == 0 and not ref.poly_mod(whole).any()


def test_encoder_impulse_response(g):
    want = [1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]  # 11 10 11 11 00 01 11
    assert g.cnav_fec_encode([1, 0, 0, 0, 0, 0, 0]).tolist() == ref.fec_encode([1, 0, 0, 0, 0, 0, 0]).tolist() == want


def test_package_encoders_against_the_restatement(g):
    rng = np.random.default_rng(3)
    for _ in range(50):
        tow, sid, tlm, flags = int(rng.integers(0, 100800)), int(rng.integers(1, 6)), int(rng.integers(0, 1 << 16)), int(rng.integers(0, 4))
        pl = list(rng.integers(0, 2, 190))
        a, b = g.lnav_subframe(tow, sid, pl, tlm=tlm, flags=flags), ref.lnav_subframe(tow, sid, pl, tlm, flags)
        assert a.dtype == np.uint8 and np.array_equal(a, b) and ref.lnav_hit(b)
        status, t, i, _, words = ref.lnav_frame(b)
        assert (status, t, i) == (0x7ff, tow, sid) and b[58] == 0 and b[59] == 0 and b[298] == 0 and b[299] == 0
        prn, mt = int(rng.integers(1, 64)), int(rng.integers(0, 64))
        pl = list(rng.integers(0, 2, 239))
        a, b = g.cnav_message(prn, mt, tow, pl), ref.cnav_message(prn, mt, tow, pl)
        assert np.array_equal(a, b) and ref.cnav_frame(b)[:4] == (3, tow, mt, prn)
        bits = rng.integers(0, 2, 77)
        assert np.array_equal(g.cnav_fec_encode(bits), ref.fec_encode(bits))


@pytest.mark.parametrize("K", [1, 3, 70])
def test_twin_trellis_lengths(env, K):
    grid.test_trellis_lengths(env, K)


def test_twin_noisy_symbols(env):
    grid.test_noisy_symbols_decode_as_sent(env)


def test_twin_degenerate_symbols(env):
    grid.test_degenerate_symbols(env)


@pytest.mark.parametrize("fmt", [ref.LNAV, ref.CNAV])
def test_twin_frame_sync(env, fmt):
    grid.test_frame_sync_grid(env, fmt)
    grid.test_frame_sync_cases(env, fmt)


def test_twin_output_subsets(env):
    grid.test_output_subsets_and_empty_capacity(env)


def test_the_python_result(g):
    rng = np.random.default_rng(4)
    bits = nc.stream_bits(rng, ref.LNAV, 137, 3, 55)
    nav = g.decode_navigation_host(nc.to_symbols(ref.LNAV, bits, inverted=True)[None, :], g.GPSL1)
    assert nav.synced.tolist() == [True] and nav.frame_offset[0] == 137 and nav.inverted[0] == 1 and nav.score[0] == 3 and nav.second_score[0] == 0
    assert nav.frames.shape == (1, 3) and nav.ok.all() and nav.tow[0].tolist() == [1000, 1001, 1002] and nav.subframe_id[0].tolist() == [1, 2, 3]
    assert nav.tow_steps[0] == 2 and nav.words.shape == (1, 3, 10) and np.array_equal(nav.bits[0], bits) and nav.path_metric.shape == (1, 1)
    cb = nc.stream_bits(rng, ref.CNAV, 83, 3, 55 + ref.TAIL)
    sym, mon = nc.rows([nc.to_symbols(ref.CNAV, cb, inverted=True, phase=1), np.zeros(7)], fill=0.0)
    nav = g.decode_navigation_host(sym, "CNAV", channels=mon)
    assert nav.synced.tolist() == [True, False] and nav.symbol_phase[0] == 1 and nav.frame_offset[0] == 83 and nav.inverted[0] == 1
    assert nav.message_type[0, :3].tolist() == [10, 11, 12] and nav.prn[0, :3].tolist() == [7, 7, 7] and nav.ok[0, :3].all() and not nav.ok[1].any()
    assert np.array_equal(nav.bits[0][:len(cb) - 8], cb[:len(cb) - 8]) and len(nav.bits[1]) == 3
    with pytest.raises(ValueError):
        g.decode_navigation_host(sym)  # bare symbols need a format


def test_every_refusal_writes_nothing(g):
    from gpuacceleratedtracking_amd import _lib
    K, cap = 3, 700
    sym = np.random.default_rng(6).standard_normal((K, cap))
    plan_fn = g.load_library().gat_nav_decode_plan

    def call(code, what, fmt=0, K=K, null_sym=False, cfg_null=False, want=nc.OUTPUTS, **fields):
        cfg = nc.config(_lib, fmt, cap, 2, 1)
        for name, v in fields.items():
            setattr(cfg, name, v)
        at, total = nc.layout(3, 0, cap, 2)  # room for the valid call's outputs: a refused call writes none of them
        buf = np.full(total, nc.CANARY, np.uint8)
        rc = g.load_library().gat_nav_decode_host(None if null_sym else sym.ctypes.data, None, K, None if cfg_null else C.byref(cfg),
                                                  *[buf.ctypes.data + at[n][0] if n in want else None for n in nc.OUTPUTS])
        assert rc == code, (what, rc)
        assert np.all(buf == nc.CANARY), what
        if not null_sym and want:  # the plan refuses the same calls (it knows no pointers)
            plan = _lib.NavPlan()
            plan.struct_size = C.sizeof(_lib.NavPlan)
            assert plan_fn(K, None if cfg_null else C.byref(cfg), C.byref(plan)) == code and plan.scratch_bytes == 0, what

    call(ARG, "null sym_re", null_sym=True)
    call(ARG, "null config", cfg_null=True)
    call(ARG, "struct_size", struct_size=C.sizeof(_lib.NavConfig) - 4)
    call(ARG, "struct_size 0", struct_size=0)
    call(ARG, "K = 0", K=0)
    call(ARG, "K < 0", K=-1)
    call(ARG, "capacity < 0", symbol_capacity=-1)
    call(ARG, "max_frames = 0", max_frames=0)
    call(ARG, "min_frames = 0", min_frames=0)
    call(ARG, "format 2", format=2)
    call(ARG, "format -1", format=-1)
    call(ARG, "every output null", want=())
    call(RANGE, "K = 4097", K=4097)
    call(RANGE, "capacity above 2^20", symbol_capacity=(1 << 20) + 1)
    call(RANGE, "scratch above 1 GiB", fmt=1, K=4096, symbol_capacity=1 << 20)
    call(RANGE, "frame workgroups", K=4096, max_frames=(1 << 31) - 1)
    # and the same call, accepted: every output is written
    rc, buf, at = nc.host_call(g, sym, None, nc.config(_lib, 0, cap, 2, 1))
    assert rc == 0 and nc.canaries_intact(buf, at) and all(not np.all(buf[o:o + n] == nc.CANARY) for o, n in at.values())
