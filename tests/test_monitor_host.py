"""The tracking monitor without a device: the package's surface; the host twin (gat_track_monitor_host) against the FP64
restatement (tests/mon_ref.py) over the whole grid -- integers equal, doubles within 1e-12 * sum|terms| (at most 2^12 terms of
2^-53 each: below 5e-13; equality is what the same order gives) --; the stream offset under a cut of the series; bit
synchronisation, C/N0 and phase lock on synthetic prompts; the forced offset; the degenerate cases; every refusal with every
output untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import mon_cases as mc
from tests import mon_ref as ref

ARG, RANGE = 1, 2
TOL = 1e-12


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def test_the_surface(g):
    """declared, bound and exported (on the parent commit none of it exists)"""
    from gpuacceleratedtracking_amd import _lib
    lib = g.load_library()
    for name in ("gat_track_monitor", "gat_track_monitor_host", "gat_track_monitor_plan"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    for name in ("monitor_accumulators", "monitor_accumulators_host", "overlay_for", "monitor_plan"):
        assert callable(getattr(g, name))
    assert callable(g.TrackingLoop.monitor)
    assert np.array_equal(g.overlay_for(g.GPSL1), np.ones(20, np.int8)) and g.overlay_for("GPSL1").dtype == np.int8
    assert np.array_equal(g.overlay_for("GPSL5"), ref.NH10) and np.array_equal(g.overlay_for("GPSL5", "pilot"), ref.NH20)
    assert "".join("0" if v > 0 else "1" for v in g.overlay_for("GPSL5", "pilot")) == "00000100110101001110"
    with pytest.raises(ValueError):
        g.overlay_for("GALE1")
    p = g.monitor_plan(97, 3, 2, 3, 1, window_blocks=7, overlay=ref.NH10)
    assert (p["num_windows"], p["search_symbols"], p["symbol_capacity"]) == (14, 8, 9) and p["scratch_bytes"] > 0


def close(a, b, scale, what):
    a, b, scale = np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(scale, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = ~(np.abs(a - b) <= TOL * scale)
    assert not bad.any(), (what, a[bad][:3], b[bad][:3])


def range_sums(x):
    c = np.concatenate([np.zeros((x.shape[0], 1)), np.cumsum(np.abs(x), axis=1)], axis=1)
    return lambda k, b0, b1: c[k, b1] - c[k, b0]


@pytest.mark.parametrize("name", list(mc.OVERLAYS))
def test_twin_against_the_restatement(g, name):
    overlay = mc.OVERLAYS[name]
    Pd = len(overlay)
    rng = np.random.default_rng(1000 + Pd + int(overlay.sum()))
    calls = 0
    for B, K, M, wt, L, l, pad in mc.data_configs(Pd):
        acc_re, acc_im, dre, dim, stride = mc.make_acc(rng, B, K, L, M, pad)
        w = mc.make_weights(rng, K, M) if wt else None
        pr, pi = ref.prompts(dre, dim, l, w)
        ar, ai = dre[:, :, l, :].astype(np.float64), dim[:, :, l, :].astype(np.float64)  # [B, K, M]
        if w is None:
            scale_r, scale_i = np.abs(ar).sum(-1).T, np.abs(ai).sum(-1).T
        else:
            scale_r = (np.abs(w.real * ar) + np.abs(w.imag * ai)).sum(-1).T
            scale_i = (np.abs(w.real * ai) + np.abs(w.imag * ar)).sum(-1).T
        E, J = ref.energies(pr, pi, overlay)
        sum_i, sum_q = range_sums(pr), range_sums(pi)
        cap = B // Pd
        win_ref = {}
        for W, fb, forced in mc.call_configs(B, Pd):
            cfg = mc.config(g, L, l, W, overlay, forced, fb)
            rc, buf, at = mc.host_call(g, acc_re, acc_im, stride, B, K, M, cfg, w)
            assert rc == 0 and mc.canaries_intact(buf, at), (B, K, M, wt, L, pad, W, fb, forced)
            calls += 1
            close(mc.take(buf, at, "prompt_re", K), pr, scale_r, "prompt_re")
            close(mc.take(buf, at, "prompt_im", K), pi, scale_i, "prompt_im")
            if W not in win_ref:
                win_ref[W] = ref.windows(pr, pi, W)
            win = mc.take(buf, at, "windows", K)
            assert win.shape == (K, (B + W - 1) // W)
            for k in range(K):
                for v, r in enumerate(win_ref[W][k]):
                    b0, b1 = v * W, min(B, (v + 1) * W)
                    assert win[k, v]["blocks"] == r["blocks"] == b1 - b0
                    close(win[k, v]["sum_p2"], r["sum_p2"], r["sum_p2"], "sum_p2")
                    close(win[k, v]["sum_p4"], r["sum_p4"], r["sum_p4"], "sum_p4")
                    close(win[k, v]["sum_d"], r["sum_d"], r["sum_p2"], "sum_d")
                    close(win[k, v]["sum_i"], r["sum_i"], sum_i(k, b0, b1), "sum_i")
                    close(win[k, v]["sum_q"], r["sum_q"], sum_q(k, b0, b1), "sum_q")
            close(mc.take(buf, at, "energy", K), E, E, "energy")
            chans = mc.take(buf, at, "channels", K)
            sre, sim, swb = (mc.take(buf, at, n, K) for n in ("sym_re", "sym_im", "sym_wbp"))
            assert sre.shape == (K, cap)
            for k in range(K):
                off, c, Jk, e_max, e_second = ref.channel(E[k], J, B, Pd, fb, forced)
                ch = chans[k]
                assert (ch["symbol_offset"], ch["start"], ch["num_symbols"], ch["reserved"]) == (off, c, Jk, 0), (B, W, fb, forced, k)
                close(ch["e_max"], e_max, e_max, "e_max")
                close(ch["e_second"], e_second, e_second, "e_second")
                if forced is None:
                    assert c == (-1 if J == 0 else int(np.argmax(E[k])))
                else:
                    assert off == forced
                rr, ri, rw = ref.symbols(pr, pi, k, c, Jk, overlay, cap)
                s_i = np.array([sum_i(k, c + j * Pd, c + (j + 1) * Pd) if j < Jk else 0.0 for j in range(cap)])
                s_q = np.array([sum_q(k, c + j * Pd, c + (j + 1) * Pd) if j < Jk else 0.0 for j in range(cap)])
                close(sre[k], rr, s_i, "sym_re")
                close(sim[k], ri, s_q, "sym_im")
                close(swb[k], rw, rw, "sym_wbp")
                assert not sre[k, Jk:].any() and not sim[k, Jk:].any() and not swb[k, Jk:].any()
    assert calls >= 1000  # 64 data configurations a block count, up to 16 calls each


def synthetic(rng, B, overlay, offset, sigma, phase=0.1, first_block=0):
    """prompts of one channel: unit amplitude, random data symbols of len(overlay) blocks starting at stream block `offset`"""
    Pd = len(overlay)
    s = first_block + np.arange(B) - offset
    data = rng.integers(0, 2, B // Pd + 3) * 2 - 1
    p = data[s // Pd + 1] * overlay[s % Pd] * np.exp(1j * phase)
    return (p + sigma * (rng.standard_normal(B) + 1j * rng.standard_normal(B)))[None, :]


def run_host(g, p, overlay, **kw):
    re, im = ref.prompts_as_acc(p)
    return g.monitor_accumulators_host(re, im, block_seconds=1e-3, prompt_index=0, overlay=overlay, **kw)


def test_stream_offset_under_a_cut(g):
    """the same series cut at first_block 0 and at 13 reports the same stream offset, and the symbols both cuts hold agree"""
    for name in ("nh10", "nh20", "ones20"):
        overlay = mc.OVERLAYS[name]
        p = synthetic(np.random.default_rng(7), 400, overlay, 13 % len(overlay), 0.3)
        a = run_host(g, p, overlay, first_block=0)
        b = run_host(g, p[:, 13:], overlay, first_block=13)
        assert a.symbol_offset[0] == b.symbol_offset[0] == 13 % len(overlay), name
        # the cut's symbols are the uncut run's from the first whole symbol of the cut on
        skip = (13 + b.start[0] - a.start[0]) // len(overlay)
        n = min(a.num_symbols[0] - skip, b.num_symbols[0])
        assert n > 10 and np.array_equal(a.symbols[0, skip:skip + n].view(np.int64), b.symbols[0, :n].view(np.int64))


@pytest.mark.parametrize("seed", range(5))
def test_bit_sync(g, seed):
    for name, offset, least in (("nh20", 13, 3.0), ("nh10", 13 % 10, 3.0), ("ones20", 7, 1.02)):
        overlay = mc.OVERLAYS[name]
        m = run_host(g, synthetic(np.random.default_rng(seed), 400, overlay, offset, 0.3), overlay)
        print(name, seed, m.symbol_offset[0], m.sync_ratio[0])
        assert m.symbol_offset[0] == offset, name
        assert m.sync_ratio[0] > least and m.synced[0], (name, m.sync_ratio[0])


@pytest.mark.parametrize("cn0", [40.0, 45.0])
def test_cn0_and_phase_lock(g, cn0):
    T, B = 1e-3, 2000
    sigma = np.sqrt(1.0 / (2.0 * T * 10.0 ** (cn0 / 10.0)))
    worst = [0.0, 0.0, 2.0]
    for seed in range(20):
        p = synthetic(np.random.default_rng(seed), B, np.ones(20, np.int8), 0, sigma)
        m = run_host(g, p, np.ones(20, np.int8), window_blocks=B, symbol_offset=0)
        assert m.cn0_m2m4.shape == (1, 1) and m.num_symbols[0] == 100
        worst = [max(worst[0], abs(m.cn0_nwpr[0] - cn0)), max(worst[1], abs(m.cn0_m2m4[0, 0] - cn0)), min(worst[2], m.phase_lock[0, 0])]
        print(cn0, seed, m.cn0_nwpr[0], m.cn0_m2m4[0, 0], m.phase_lock[0, 0])
        assert abs(m.cn0_nwpr[0] - cn0) <= 0.3, (seed, m.cn0_nwpr[0])
        assert abs(m.cn0_m2m4[0, 0] - cn0) <= 0.5, (seed, m.cn0_m2m4[0, 0])
        assert m.phase_lock[0, 0] > 0.85
        # the figures are the restatement's, from the same raw sums
        w = m.windows[0, 0]
        assert abs(ref.cn0_m2m4(w, T) - m.cn0_m2m4[0, 0]) < 1e-9
        assert abs(ref.cn0_nwpr(m.symbols[0].real, m.symbols[0].imag, m.wbp[0], 100, 20, T) - m.cn0_nwpr[0]) < 1e-9
    print("worst", cn0, worst)


def test_a_rotating_prompt_has_no_phase_lock(g):
    p = np.exp(2j * np.pi * 200.0 * 1e-3 * np.arange(400))[None, :]
    m = run_host(g, p, np.ones(20, np.int8), window_blocks=400)
    assert abs(m.phase_lock[0, 0]) < 1e-6
    locked = run_host(g, np.full((1, 400), np.exp(0.1j)), np.ones(20, np.int8), window_blocks=400)
    assert abs(locked.phase_lock[0, 0] - np.cos(0.2)) < 1e-6


def test_forced_offset_gives_the_searched_symbols(g):
    overlay = ref.NH10
    p = synthetic(np.random.default_rng(3), 97, overlay, 6, 0.3, first_block=13)
    a = run_host(g, p, overlay, first_block=13)
    b = run_host(g, p, overlay, first_block=13, symbol_offset=int(a.symbol_offset[0]))
    assert a.symbol_offset[0] == b.symbol_offset[0] == 6 and a.start[0] == b.start[0] == (6 - 13) % 10
    for x, y in ((a.symbols, b.symbols), (a.wbp, b.wbp), (a.energy, b.energy)):
        assert np.array_equal(np.ascontiguousarray(x).view(np.int64), np.ascontiguousarray(y).view(np.int64))
    assert np.array_equal(a.bits, b.bits) and set(np.unique(a.bits[0, :a.num_symbols[0]])) <= {-1, 1}
    other = run_host(g, p, overlay, first_block=13, symbol_offset=7)
    assert other.symbol_offset[0] == 7 and other.sync_ratio[0] < 1.0 and not other.synced[0]


def test_degenerate_cases(g):
    rng = np.random.default_rng(5)
    for Pd in (2, 10, 20):
        for B in range(1, 2 * Pd - 1):
            m = run_host(g, synthetic(rng, B, np.ones(Pd, np.int8), 0, 0.1), np.ones(Pd, np.int8))
            assert m.start[0] == -1 and m.symbol_offset[0] == -1 and m.num_symbols[0] == 0 and not m.synced[0]
            assert not m.energy.any() and not m.symbols.any() and m.channels["e_max"][0] == 0.0 and np.isnan(m.cn0_nwpr[0])
        m = run_host(g, synthetic(rng, 2 * Pd - 1, np.ones(Pd, np.int8), 0, 0.1), np.ones(Pd, np.int8))
        assert m.start[0] >= 0 and m.num_symbols[0] >= 1
    p = synthetic(rng, 37, np.ones(1, np.int8), 0, 0.1)
    m = run_host(g, p, np.ones(1, np.int8), keep_prompts=True)
    assert m.start[0] == 0 and m.symbol_offset[0] == 0 and m.num_symbols[0] == 37 and m.channels["e_second"][0] == 0.0
    assert np.array_equal(m.symbols.view(np.int64), m.prompts.view(np.int64)) and np.isnan(m.cn0_nwpr[0])
    assert np.array_equal(m.prompts.astype(np.complex64), p.astype(np.complex64))


def test_every_refusal_writes_nothing(g):
    B, K, L, M, W, Pd = 24, 2, 3, 2, 7, 10
    rng = np.random.default_rng(11)
    acc_re, acc_im, _, _, stride = mc.make_acc(rng, B, K, L, M, 0)
    w = mc.make_weights(rng, K, M)
    w_re, w_im = np.ascontiguousarray(w.real), np.ascontiguousarray(w.imag)
    fn = g.load_library().gat_track_monitor_host
    at, total = mc.layout(B, K, Pd, W)

    def call(code, what, acc=(True, True), stride=stride, B=B, K=K, M=M, wts=(None, None), want=mc.OUTPUTS, cfg_null=False, **fields):
        cfg = mc.config(g, L, 1, W, ref.NH10, None, 0)
        for name, v in fields.items():
            if name == "overlay3":
                cfg.overlay[3] = v
            else:
                setattr(cfg, name, v)
        buf = np.full(total, mc.CANARY)
        rc = mc.raw_call(fn, None, acc_re.ctypes.data if acc[0] else None, acc_im.ctypes.data if acc[1] else None, stride, B, K, M,
                         None if cfg_null else cfg, wts[0], wts[1], buf.ctypes.data, {n: at[n] for n in want})
        assert rc == code, (what, rc)
        assert np.all(buf == mc.CANARY), what

    call(ARG, "null acc_re", acc=(False, True))
    call(ARG, "null acc_im", acc=(True, False))
    call(ARG, "null config", cfg_null=True)
    call(ARG, "struct_size", struct_size=C.sizeof(g.monitor._lib.MonitorConfig) - 8)
    call(ARG, "struct_size 0", struct_size=0)
    call(ARG, "B = 0", B=0)
    call(ARG, "B < 0", B=-1)
    call(ARG, "K = 0", K=0)
    call(ARG, "M = 0", M=0)
    call(ARG, "L = 0", num_taps=0, prompt_index=0)
    call(RANGE, "M = 65", M=65, stride=K * L * 65)
    call(RANGE, "B > 2^20", B=(1 << 20) + 1)
    call(RANGE, "K = 4097", K=4097, stride=4097 * L * M)
    call(RANGE, "prompt_index = L", prompt_index=L)
    call(RANGE, "prompt_index < 0", prompt_index=-1)
    call(ARG, "W = 0", window_blocks=0)
    call(RANGE, "Pd = 0", symbol_blocks=0)
    call(RANGE, "Pd = 129", symbol_blocks=129)
    call(ARG, "overlay entry 0", overlay3=0)
    call(ARG, "overlay entry 2", overlay3=2)
    call(RANGE, "symbol_offset = -2", symbol_offset=-2)
    call(RANGE, "symbol_offset = Pd", symbol_offset=Pd)
    call(ARG, "first_block < 0", first_block=-1)
    call(ARG, "stride below a block", stride=K * L * M - 1)
    call(ARG, "negative stride", stride=-stride)
    call(ARG, "w_re alone", wts=(w_re.ctypes.data, None))
    call(ARG, "w_im alone", wts=(None, w_im.ctypes.data))
    call(ARG, "every output null", want=())
    # and the same call, accepted: every output is written, one block takes any stride
    cfg = mc.config(g, L, 1, W, ref.NH10, None, 0)
    rc, buf, at2 = mc.host_call(g, acc_re, acc_im, stride, B, K, M, cfg, w)
    assert rc == 0 and mc.canaries_intact(buf, at2) and all(not np.any(buf[o:o + n] == mc.CANARY) for o, n in at2.values())
    rc, buf, at2 = mc.host_call(g, acc_re, acc_im, -5, 1, K, M, cfg, w)
    assert rc == 0 and mc.canaries_intact(buf, at2)


def test_the_pipeline_tests_expected_bias_is_the_measured_one(g):
    """the constants tests/test_monitor_pipeline_gpu.py expects its C/N0 figures around (tests/mon_cases.py), measured again: the
    twin's figures on the 20 seeds (the twin is the restatement to 1e-12, above)"""
    for (sat, frac), want in mc.PIPELINE_EXPECTED.items():
        d = []
        for seed in range(20):
            p = mc.edge_series(mc.PIPELINE_BITS[sat], mc.PIPELINE_SKIP, mc.PIPELINE_BLOCKS, frac, mc.PIPELINE_CN0, 1e-3, np.random.default_rng(seed))
            pr, pi = np.ascontiguousarray(p.real), np.ascontiguousarray(p.imag)
            E, J = ref.energies(pr, pi, np.ones(20, np.int8)) if seed == 0 else (None, None)
            m = g.monitor_accumulators_host(p.real.T[:, :, None, None], p.imag.T[:, :, None, None], block_seconds=1e-3, prompt_index=0,
                                            first_block=mc.PIPELINE_SKIP, window_blocks=mc.PIPELINE_BLOCKS)
            if seed == 0:  # one seed through the restatement itself
                assert np.allclose(m.energy, E, rtol=1e-5) and m.start[0] == ref.channel(E[0], J, mc.PIPELINE_BLOCKS, 20, mc.PIPELINE_SKIP)[1]
            assert m.symbol_offset[0] == (0 if frac < 0.5 else 19) and m.sync_ratio[0] > 1.02
            d.append((m.cn0_nwpr[0] - mc.PIPELINE_CN0, m.cn0_m2m4[0, 0] - mc.PIPELINE_CN0))
        d = np.array(d)
        got = (d[:, 0].mean(), np.abs(d[:, 0] - d[:, 0].mean()).max(), d[:, 1].mean(), np.abs(d[:, 1] - d[:, 1].mean()).max())
        print(sat, frac, got)
        assert np.allclose(got, want, atol=0.005), (sat, frac, got)
