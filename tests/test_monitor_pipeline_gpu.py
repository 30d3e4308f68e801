"""The receiver end to end with the tracking monitor behind the loop: a noisy two-satellite GPS L1 C/A stream with data bits,
``TrackingLoop.run`` over 400 blocks, ``loop.monitor`` on the accumulators it left on the device -- where the bit edges are, what
the bits are, whether the carrier loop is locked and how strong the satellites are.

fs = 4 MHz, N = 4000 (1 ms), M = 2; 440 generator blocks; a data bit is 20 generator blocks and is put in as a half cycle added to
the block's carrier phase, which is otherwise continuous; the noise sets M fs / (2 sigma^2) = 43 dB-Hz.  The receiver starts N/4 or
3N/4 into the generator's stream, so every bit edge falls inside receiver block 19 mod 20: three quarters old bit in the first
case (the symbol starts at block 0), three quarters new bit in the second (it starts at block 19).

Both C/N0 estimators read low with a bit edge inside a block.  The expected distance from 43 dB-Hz and the 20-seed spread are
measured on the FP64 restatement with synthetic prompts of the same blocks, edge position, bits and C/N0 (tests/mon_cases.py
PIPELINE_EXPECTED, about -1 dB; tests/test_monitor_host.py measures them again); the loop may lose 0.5 dB more (at 18 Hz and 43 dB-Hz
its phase jitter costs under 0.01 dB)."""
import numpy as np
import pytest

from tests import mon_cases as mc
from tests import mon_ref as ref

pytestmark = pytest.mark.gpu

N, M, FS, FC = 4000, 2, 4e6, 1.023e6
T = N / FS
PRNS = np.array([7, 19])
DOP = np.array([-2210.0, 310.0])
TAU0 = np.array([511.9, 100.3])
PHI0 = np.array([0.6, 0.1])
GEN_BLOCKS, RUN_BLOCKS = 440, 400


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def make_stream(g, noise_sigma, blocks=GEN_BLOCKS):
    system = g.GPSL1()
    fcode = FC * (1 + DOP / 1575.42e6)
    b = np.arange(blocks, dtype=np.float64)[:, None]
    tau = np.mod(TAU0[None, :] + fcode[None, :] * T * b, 1023.0)
    bits = np.stack([np.repeat(x, 20)[:blocks] for x in mc.PIPELINE_BITS], axis=1)  # [blocks, K]
    phi = np.mod(PHI0[None, :] + DOP[None, :] * T * b + 0.25 * (1 - bits), 1.0)   # a half cycle where the bit is -1
    prm = g.make_params(PRNS - 1, fcode, DOP, tau, 2 * np.pi * phi, shape=(blocks, PRNS.size))
    re, im = g.gen_signal_stream(system, prm, FS, N, M, noise_sigma=noise_sigma, seed=2024)
    return system, fcode, re, im


def make_loop(g, system, fcode, start, **kw):
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), FS, 0.5)
    # handed over as an acquisition with a fine-frequency stage would: 0.2 Hz, 0.02 chip and 0.02 cycle off, so that the 40 blocks
    # skipped in front hold the whole transient (a 3 Hz error takes the 18 Hz loop through 30 degrees for 200 ms)
    return g.TrackingLoop(system, PRNS, N, M, FS, shifts, init_carrier_doppler=DOP + 0.2, init_code_phase=TAU0 + fcode * start / FS + 0.02,
                          init_carrier_phase=np.mod(PHI0 + DOP * start / FS + 0.02, 1.0), dll_bandwidth_hz=4.0, **kw)


@pytest.fixture(scope="module")
def stream(g):
    sigma = np.sqrt(M * FS / (2.0 * 10.0 ** (mc.PIPELINE_CN0 / 10.0)))
    return make_stream(g, sigma)


@pytest.mark.parametrize("frac", [0.25, 0.75])
def test_receiver_end_to_end(g, stream, frac):
    system, fcode, re, im = stream
    start = int(frac * N)
    loop = make_loop(g, system, fcode, start)
    acc_re, acc_im = loop.run(re, im, RUN_BLOCKS, start=start, keep=True)
    skip, B = mc.PIPELINE_SKIP, mc.PIPELINE_BLOCKS
    assert RUN_BLOCKS - skip == B
    mon = loop.monitor(acc_re[skip:], acc_im[skip:], first_block=skip)             # windows of 20 blocks
    whole = loop.monitor(acc_re[skip:], acc_im[skip:], first_block=skip, window_blocks=B)
    loop.ctx.sync()
    offset = 0 if frac < 0.5 else 19
    print("offset", mon.symbol_offset, "ratio", mon.sync_ratio, "lock", mon.phase_lock.min(axis=1), "nwpr", mon.cn0_nwpr, "m2m4", whole.cn0_m2m4[:, 0])
    assert list(mon.symbol_offset) == [offset, offset] and list(mon.start) == [(offset - skip) % 20] * 2
    assert mon.synced.all() and whole.synced.all()
    # the bits, up to the Costas loop's one sign per channel: symbol j starts at stream block skip + start + 20 j
    nsym = (B - int(mon.start[0])) // 20
    first_bit = (skip + int(mon.start[0]) + 1) // 20 if offset else skip // 20
    assert list(mon.num_symbols) == [nsym, nsym] and nsym >= 17
    for k in range(2):
        sent = mc.PIPELINE_BITS[k][first_bit:first_bit + nsym]
        got = mon.bits[k, :nsym]
        assert np.array_equal(got, sent) or np.array_equal(got, -sent), (k, got, sent)
        assert not mon.bits[k, nsym:].any()
    assert mon.phase_lock.shape == (2, B // 20) and (mon.phase_lock > 0.8).all(), mon.phase_lock
    # the figures are the restatement's from the same accumulators copied back
    h_re, h_im = acc_re[skip:].cpu().numpy(), acc_im[skip:].cpu().numpy()
    r = ref.monitor(h_re, h_im, int(loop.config.prompt_index), B, np.ones(20, np.int8), first_block=skip)
    for k in range(2):
        off, c, Jk, e_max, e_second = r["channels"][k]
        assert (off, c, Jk) == (mon.symbol_offset[k], mon.start[k], mon.num_symbols[k])
        assert abs(ref.cn0_nwpr(r["sym_re"][k], r["sym_im"][k], r["sym_wbp"][k], Jk, 20, T) - mon.cn0_nwpr[k]) < 1e-9
        assert abs(ref.cn0_m2m4(r["windows"][k][0], T) - whole.cn0_m2m4[k, 0]) < 1e-9
        assert abs(ref.phase_lock(r["windows"][k][0]) - whole.phase_lock[k, 0]) < 1e-12
        # and lie where the restatement puts them for this edge position: its bias, its 20-seed spread and 0.5 dB of tracking loss
        b_nwpr, s_nwpr, b_m2m4, s_m2m4 = mc.PIPELINE_EXPECTED[(k, frac)]
        assert abs(mon.cn0_nwpr[k] - (mc.PIPELINE_CN0 + b_nwpr)) <= s_nwpr + 0.5, (k, mon.cn0_nwpr[k])
        assert abs(whole.cn0_m2m4[k, 0] - (mc.PIPELINE_CN0 + b_m2m4)) <= s_m2m4 + 0.5, (k, whole.cn0_m2m4[k, 0])


def test_the_beamformed_loops_monitor_uses_its_weights(g):
    """TrackingLoop(weights=...): the monitor's prompt is sum_m conj(w) acc of the loop's own weights"""
    system, fcode, re, im = make_stream(g, 0.0, blocks=64)
    w = np.array([[0.6 + 0.1j, 0.4 - 0.1j], [0.3 - 0.2j, 0.7 + 0.2j]])
    loop = make_loop(g, system, fcode, 0, weights=w)
    acc_re, acc_im = loop.run(re, im, 60, keep=True)
    mon = loop.monitor(acc_re, acc_im, keep_prompts=True)
    plain = loop.monitor(acc_re, acc_im, keep_prompts=True, weights=None)
    loop.ctx.sync()
    acc = acc_re.cpu().numpy().astype(np.float64) + 1j * acc_im.cpu().numpy().astype(np.float64)   # [B, K, L, M]
    tap = acc[:, :, int(loop.config.prompt_index), :]
    want = np.einsum("km,bkm->kb", np.conj(w), tap)
    scale = np.einsum("km,bkm->kb", np.abs(w), np.abs(tap))
    assert mon.prompts.shape == (2, 60) and np.all(np.abs(mon.prompts - want) <= 1e-12 * scale)
    assert np.all(np.abs(plain.prompts - tap.sum(-1).T) <= 1e-12 * np.abs(tap).sum(-1).T) and not np.allclose(plain.prompts, mon.prompts)
