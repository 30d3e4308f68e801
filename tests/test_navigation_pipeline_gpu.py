"""The navigation data layer behind the monitor, on the device from accumulators to frames.

(a) Synthetic accumulators [B, K, 1, 1] made from LNAV bits (twenty blocks a bit) and from CNAV symbols under the NH10 overlay (ten
blocks a symbol) with noise go through ``monitor_accumulators`` and then ``decode_navigation``, which takes the monitor's device
tensors as they are -- nothing is read back in between --: the frames, the polarity and the TOW counts come out as sent, a channel
whose prompts were negated included.

(b) End to end with the correlator: two GPS L1 satellites, one antenna, fs = 2.046 MHz, N = 2046 (1 ms), 45 dB-Hz; 620 data bits
(13 junk, two subframes with consecutive TOW, 7 junk) put in as half cycles of carrier phase, as tests/test_monitor_pipeline_gpu.py
does; ``TrackingLoop.run`` over the 12400 blocks, ``loop.monitor``, ``loop.navigation``: both subframes come out with all ten
words' parity good, the sent TOWs and one TOW step, and ``inverted`` is the sign the monitor's bits show against the sent bits."""
import numpy as np
import pytest

from tests import nav_cases as nc
from tests import nav_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def accumulators(rng, symbols_pm, overlay, lead, sigma, negate):
    """float32 [B, K, 1, 1] planes: the last `lead` blocks of a +1 symbol, then every symbol of the channel over the overlay, then
    noise; unit amplitude at a phase of 0.15 rad, negated where the Costas loop locked to the negative"""
    K, Pd = len(symbols_pm), len(overlay)
    B = lead + Pd * max(len(s) for s in symbols_pm) + 3
    p = np.zeros((B, K), np.complex128)
    for k, s in enumerate(symbols_pm):
        series = np.concatenate([overlay[Pd - lead:], (np.asarray(s, np.float64)[:, None] * overlay[None, :]).reshape(-1)])
        p[:len(series), k] = series * np.exp(0.15j) * (-1.0 if negate[k] else 1.0)
    p += sigma * (rng.standard_normal(p.shape) + 1j * rng.standard_normal(p.shape))
    return np.ascontiguousarray(p.real[:, :, None, None], np.float32), np.ascontiguousarray(p.imag[:, :, None, None], np.float32)


@pytest.mark.parametrize("fmt", [ref.LNAV, ref.CNAV])
def test_monitor_to_frames_on_the_device(g, fmt):
    import torch

    rng = np.random.default_rng(70 + fmt)
    K, negate = 3, [False, True, False]
    prefixes = [13, 137, 0]
    tail = ref.TAIL + 8 if fmt == ref.CNAV else 7
    bits = [nc.stream_bits(rng, fmt, prefixes[k], 2, tail, tow0=5000 + 10 * k) for k in range(K)]
    symbols = [1.0 - 2.0 * (ref.fec_encode(b) if fmt == ref.CNAV else b).astype(np.float64) for b in bits]
    overlay = g.overlay_for("GPSL5" if fmt == ref.CNAV else "GPSL1").astype(np.float64)
    lead = 7
    acc_re, acc_im = accumulators(rng, symbols, overlay, lead, 0.7, negate)
    mon = g.monitor_accumulators(torch.from_numpy(acc_re).cuda(), torch.from_numpy(acc_im).cuda(), block_seconds=1e-3, prompt_index=0,
                                 overlay=overlay)
    nav = g.decode_navigation(mon)  # the format from the monitor's symbol length; the monitor's tensors, not copies
    assert mon._host is None, "the monitor was read back before the decoder ran"
    assert nav.format == fmt and list(mon.symbol_offset) == [lead] * K
    print("offset", nav.frame_offset, "inverted", nav.inverted, "score", nav.score, nav.second_score, "tow", nav.tow[:, :2].tolist())
    assert nav.synced.all() and list(nav.frame_offset) == prefixes and list(nav.inverted) == [int(v) for v in negate]
    assert list(nav.symbol_phase) == [0] * K and list(nav.score) == [2] * K and list(nav.second_score) == [0] * K
    assert list(nav.num_frames) == [2] * K and list(nav.tow_steps) == [1] * K and nav.ok[:, :2].all() and not nav.status[:, 2:].any()
    for k in range(K):
        assert nav.tow[k, :2].tolist() == [5000 + 10 * k, 5001 + 10 * k]
        sent = bits[k][:len(bits[k]) - (ref.TAIL if fmt == ref.CNAV else 0)]
        assert np.array_equal(nav.bits[k][:len(sent)], sent), k
        want = [ref.cnav_frame(bits[k][prefixes[k] + 300 * f:][:300]) if fmt == ref.CNAV else ref.lnav_frame(bits[k][prefixes[k] + 300 * f:][:300])
                for f in range(2)]
        assert [[int(w) for w in nav.words[k, f]] for f in range(2)] == [w[4] for w in want]
        assert nav.subframe_id[k, :2].tolist() == [w[2] for w in want] and nav.prn[k, :2].tolist() == [w[3] for w in want]
    # the twin on the monitor's symbols read back: the same records and frames
    host = g.decode_navigation_host(mon)
    assert np.array_equal(host.channels, nav.channels) and np.array_equal(host.frames, nav.frames) and np.array_equal(host.decoded, nav.decoded)
    assert np.array_equal(host.path_metric, nav.path_metric)


N, M, FS, FC = 2046, 1, 2.046e6, 1.023e6
T = N / FS
PRNS = np.array([7, 19])
DOP = np.array([-2210.0, 310.0])
TAU0 = np.array([511.9, 100.3])
PHI0 = np.array([0.6, 0.1])
CN0 = 45.0
TOW0 = (40123, 100799)  # the second satellite's count rolls over at the end of the week


def test_receiver_end_to_end(g):
    rng = np.random.default_rng(11)
    sent = [np.concatenate([nc.junk(rng, 13), nc.lnav_frames(rng, 2, tow0=TOW0[k]), nc.junk(rng, 7)]) for k in range(2)]
    assert all(len(b) == 620 for b in sent)
    blocks = 620 * 20
    system = g.GPSL1()
    fcode = FC * (1 + DOP / 1575.42e6)
    b = np.arange(blocks, dtype=np.float64)[:, None]
    tau = np.mod(TAU0[None, :] + fcode[None, :] * T * b, 1023.0)
    half = np.stack([np.repeat(x, 20) for x in sent], axis=1).astype(np.float64)  # [blocks, K]: a 1 bit is a half cycle
    phi = np.mod(PHI0[None, :] + DOP[None, :] * T * b + 0.5 * half, 1.0)
    prm = g.make_params(PRNS - 1, fcode, DOP, tau, 2 * np.pi * phi, shape=(blocks, PRNS.size))
    re, im = g.gen_signal_stream(system, prm, FS, N, M, noise_sigma=float(np.sqrt(M * FS / (2.0 * 10.0 ** (CN0 / 10.0)))), seed=2025)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), FS, 0.5)
    loop = g.TrackingLoop(system, PRNS, N, M, FS, shifts, init_carrier_doppler=DOP + 0.2, init_code_phase=TAU0 + 0.02,
                          init_carrier_phase=np.mod(PHI0 + 0.02, 1.0), dll_bandwidth_hz=4.0)
    acc_re, acc_im = loop.run(re, im, blocks, keep=True)
    mon = loop.monitor(acc_re, acc_im)
    nav = loop.navigation(mon)
    assert mon._host is None and nav.format == 0
    print("symbol offset", mon.symbol_offset, "lock", mon.phase_lock.min(axis=1), "frame offset", nav.frame_offset, "inverted", nav.inverted,
          "score", nav.score, nav.second_score, "tow", nav.tow.tolist(), "status", nav.status.tolist())
    assert list(mon.symbol_offset) == [0, 0] and list(mon.num_symbols) == [620, 620]
    assert nav.synced.all() and list(nav.frame_offset) == [13, 13] and list(nav.num_frames) == [2, 2] and list(nav.score) == [2, 2]
    assert (nav.status == 0x7ff).all() and list(nav.tow_steps) == [1, 1]
    for k in range(2):
        assert nav.tow[k].tolist() == [TOW0[k], (TOW0[k] + 1) % 100800] and nav.subframe_id[k].tolist() == [1, 2]
        got, want = mon.bits[k, 13:], 1 - 2 * sent[k][13:].astype(np.int64)  # from the first subframe on (the junk covers the transient)
        flipped = bool(np.array_equal(got, -want))
        assert flipped or np.array_equal(got, want), k
        assert nav.inverted[k] == int(flipped)
        assert np.array_equal(nav.bits[k][13:], sent[k][13:])
