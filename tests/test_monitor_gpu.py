"""GPU tests of the tracking monitor (include/gat.h gat_track_monitor; csrc/gat_mon.hip).

Every output of the device call lies in ONE flat buffer between canaries (tests/mon_cases.py) and is compared with the host twin's
buffer as integer views: every output bit for bit and every canary intact in one comparison, over the grid of
tests/test_monitor_host.py (which holds the twin to the FP64 restatement on the CPU).  The accumulators carry NaN between the
blocks, so a finite result shows the padding is not read.  Subsets of the outputs, shapes beyond one workgroup of every kernel,
the same call twice, the refusals and the Python surface follow.  The call does not synchronise: results are read after
ctx.sync() only."""
import numpy as np
import pytest

from tests import mon_cases as mc
from tests import mon_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


class Device:
    """the accumulators and weights of one data configuration on the device, and calls on them"""

    def __init__(self, g, acc_re, acc_im, stride, B, K, M, w=None):
        import torch
        self.g, self.ctx, self.torch = g, g.get_context(), torch
        dev = self.ctx.device
        self.re, self.im = torch.from_numpy(acc_re).to(dev), torch.from_numpy(acc_im).to(dev)
        self.w = None if w is None else (torch.from_numpy(np.ascontiguousarray(w.real)).to(dev), torch.from_numpy(np.ascontiguousarray(w.imag)).to(dev))
        self.stride, self.B, self.K, self.M = stride, B, K, M

    def enqueue(self, cfg, want=mc.OUTPUTS):
        """the call, not synchronised: (status, device buffer, layout)"""
        at, total = mc.layout(self.B, self.K, int(cfg.symbol_blocks), int(cfg.window_blocks), want)
        buf = self.torch.full((total,), mc.CANARY, dtype=self.torch.float64, device=self.ctx.device)
        rc = mc.raw_call(self.ctx.lib.gat_track_monitor, self.ctx._h, self.re.data_ptr(), self.im.data_ptr(), self.stride, self.B, self.K, self.M, cfg,
                         self.w[0].data_ptr() if self.w else None, self.w[1].data_ptr() if self.w else None, buf.data_ptr(), at)
        return rc, buf, at


def same_bits(dev_buf, host_buf):
    a = dev_buf.cpu().numpy()
    return a.shape == host_buf.shape and np.array_equal(a.view(np.int64), host_buf.view(np.int64))


@pytest.mark.parametrize("name", list(mc.OVERLAYS))
def test_device_equals_the_twin_bit_for_bit(g, name):
    overlay = mc.OVERLAYS[name]
    Pd = len(overlay)
    rng = np.random.default_rng(2000 + Pd + int(overlay.sum()))
    calls = 0
    for B, K, M, wt, L, l, pad in mc.data_configs(Pd):
        acc_re, acc_im, _, _, stride = mc.make_acc(rng, B, K, L, M, pad)
        w = mc.make_weights(rng, K, M) if wt else None
        d = Device(g, acc_re, acc_im, stride, B, K, M, w)
        pending = []
        for W, fb, forced in mc.call_configs(B, Pd):
            cfg = mc.config(g, L, l, W, overlay, forced, fb)
            rc, buf, at = d.enqueue(cfg)
            assert rc == 0, (B, K, M, wt, L, pad, W, fb, forced)
            pending.append((cfg, buf, (W, fb, forced)))
        d.ctx.sync()
        for cfg, buf, what in pending:
            rc, host, at = mc.host_call(g, acc_re, acc_im, stride, B, K, M, cfg, w)
            assert rc == 0 and mc.canaries_intact(host, at) and mc.outputs_finite(host, at, K), (B, K, M, wt, L, pad, what)
            assert same_bits(buf, host), (B, K, M, wt, L, pad, what)
            calls += 1
    assert calls >= 1000


SUBSETS = [("windows",), ("sym_re", "sym_im", "sym_wbp"), ("channels",), ("energy",), ("prompt_re",), ("prompt_im", "sym_wbp"), ("sym_re",),
           ("windows", "channels"), ("prompt_re", "prompt_im", "energy", "channels")]


def test_null_subsets_of_the_outputs(g):
    rng = np.random.default_rng(31)
    B, K, L, M, pad = 97, 3, 3, 3, 5
    acc_re, acc_im, _, _, stride = mc.make_acc(rng, B, K, L, M, pad)
    w = mc.make_weights(rng, K, M)
    d = Device(g, acc_re, acc_im, stride, B, K, M, w)
    for overlay, forced in ((ref.NH10, None), (ref.NH20, 4)):
        cfg = mc.config(g, L, 1, 7, overlay, forced, 13)
        pending = [(want, d.enqueue(cfg, want)) for want in SUBSETS]
        d.ctx.sync()
        for want, (rc, buf, at) in pending:
            hrc, host, at = mc.host_call(g, acc_re, acc_im, stride, B, K, M, cfg, w, want)
            assert rc == 0 and hrc == 0 and mc.outputs_finite(host, at, K), want
            assert same_bits(buf, host), want


@pytest.mark.parametrize("B,K,M,Pd,W", [(4099, 5, 2, 20, 20), (4099, 5, 2, 20, 4099), (4099, 5, 2, 20, 1), (45, 300, 1, 2, 3)])
def test_beyond_one_workgroup_of_every_kernel(g, B, K, M, Pd, W):
    """4099 x 5: prompts, windows (one wave each; W = 4099: 65 trips of one wave), terms and symbols over many workgroups;
    300 channels: the energies and the choice too"""
    rng = np.random.default_rng(B + K)
    L = 3
    acc_re, acc_im, _, _, stride = mc.make_acc(rng, B, K, L, M, 3)
    overlay = ref.NH20 if Pd == 20 else mc.OVERLAYS["pd2"]
    plan = g.monitor_plan(B, K, M, L, 1, W, overlay, acc_block_stride=stride)
    if K == 300:
        assert plan["energy_workgroups"] > 1 and plan["pick_workgroups"] > 1
    else:
        assert min(plan[n] for n in ("prompt_workgroups", "window_workgroups", "term_workgroups", "symbol_workgroups")) > 1
    w = mc.make_weights(rng, K, M)
    d = Device(g, acc_re, acc_im, stride, B, K, M, w)
    cfg = mc.config(g, L, 1, W, overlay, None, 13)
    rc, buf, at = d.enqueue(cfg)
    rc2, buf2, _ = d.enqueue(cfg)  # the same call twice: the same bits
    d.ctx.sync()
    hrc, host, at = mc.host_call(g, acc_re, acc_im, stride, B, K, M, cfg, w)
    assert rc == 0 and rc2 == 0 and hrc == 0 and mc.outputs_finite(host, at, K)
    assert same_bits(buf, host) and same_bits(buf2, host)


def test_refusals_write_nothing(g):
    rng = np.random.default_rng(41)
    B, K, L, M = 24, 2, 3, 2
    acc_re, acc_im, _, _, stride = mc.make_acc(rng, B, K, L, M, 0)
    d = Device(g, acc_re, acc_im, stride, B, K, M)
    cases = [(dict(window_blocks=0), 1), (dict(symbol_blocks=129), 2), (dict(prompt_index=3), 2), (dict(symbol_offset=10), 2), (dict(first_block=-1), 1),
             (dict(struct_size=8), 1)]
    pending = []
    for fields, code in cases:
        cfg = mc.config(g, L, 1, 7, ref.NH10, None, 0)
        at, total = mc.layout(B, K, 10, 7)
        for n, v in fields.items():
            setattr(cfg, n, v)
        buf = d.torch.full((total,), mc.CANARY, dtype=d.torch.float64, device=d.ctx.device)
        rc = mc.raw_call(d.ctx.lib.gat_track_monitor, d.ctx._h, d.re.data_ptr(), d.im.data_ptr(), stride, B, K, M, cfg, None, None, buf.data_ptr(), at)
        assert rc == code, fields
        assert d.ctx.lib.gat_last_error(d.ctx._h), fields
        pending.append(buf)
    d.stride = stride - 1
    rc, buf, _ = d.enqueue(mc.config(g, L, 1, 7, ref.NH10, None, 0))
    assert rc == 1
    d.ctx.sync()
    for b in pending + [buf]:
        assert bool((b == mc.CANARY).all())


def test_the_python_surface(g):
    """monitor_accumulators on a padded device tensor against monitor_accumulators_host: the same raw sums, the same figures"""
    import torch
    rng = np.random.default_rng(51)
    B, K, L, M = 203, 3, 3, 2
    T = 1e-3
    sigma = np.sqrt(1.0 / (2.0 * T * 10.0 ** 5.0))  # 50 dB-Hz: nine symbols place the bit edge
    p = np.stack([np.repeat(rng.integers(0, 2, B // 20 + 2) * 2 - 1, 20)[7 - k:7 - k + B] * np.exp(0.1j * k) for k in range(K)])
    acc = rng.standard_normal((B, K, L, M)) + 1j * rng.standard_normal((B, K, L, M))
    acc[:, :, 1, :] = (p.T[:, :, None] / M) + sigma * (rng.standard_normal((B, K, M)) + 1j * rng.standard_normal((B, K, M))) / np.sqrt(M)
    w = mc.make_weights(rng, K, M)
    dev = g.get_context().device
    big = torch.full((B, K * L * M + 6), float("nan"), dtype=torch.float32, device=dev)
    big_im = big.clone()
    big[:, :K * L * M] = torch.from_numpy(acc.real.reshape(B, -1).astype(np.float32)).to(dev)
    big_im[:, :K * L * M] = torch.from_numpy(acc.imag.reshape(B, -1).astype(np.float32)).to(dev)
    acc_re, acc_im = (t.as_strided((B, K, L, M), (K * L * M + 6, L * M, M, 1)) for t in (big, big_im))
    for weights in (None, w):
        kw = dict(block_seconds=T, prompt_index=1, window_blocks=50, first_block=33, weights=weights, keep_prompts=True)
        m = g.monitor_accumulators(acc_re, acc_im, **kw)
        h = g.monitor_accumulators_host(acc.real.astype(np.float32), acc.imag.astype(np.float32), **kw)
        for name in ("phase_lock", "cn0_m2m4", "symbol_offset", "start", "num_symbols", "sync_ratio", "synced", "bits", "cn0_nwpr", "energy", "wbp"):
            a, b = getattr(m, name), getattr(h, name)
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), name
        assert np.array_equal(m.symbols, h.symbols) and np.array_equal(m.prompts, h.prompts)
        assert m.phase_lock.shape == (K, 5) and m.bits.shape == (K, 10) and m.bits.dtype == np.int8
        if weights is None:
            assert list(m.symbol_offset) == [(33 + k - 7) % 20 for k in range(K)] and np.isfinite(m.cn0_nwpr).all()
