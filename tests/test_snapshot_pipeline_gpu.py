"""The snapshot fix in its two chains, on device tensors with nothing read back in between.

Chain 1: ``snapshot_fix`` -> ``position_fix_raim`` -> ``range_corrections`` -> ``velocity_fix``: the whole milliseconds the snapshot
fix resolves, the caller's fractions, the reception it hands on and the caller's ``rx_frac`` go into every existing back-end call as
they are; the records of every stage equal the bytes of the same chain through the host twins.

Chain 2: acquisition to position.  One block of 1 ms at 20 MHz with the eight satellites of fix_cases' ``short`` case at the code
phases and Dopplers of its first epoch, no noise; ``acquire(method="fft")`` at sample spacing -> ``code_fractions`` ->
``snapshot_fix``.  Byte-equal to the twin fed the same fractions.  Against the truth: the search's code phase is the true one
rounded to the sample, so every range is off by at most c / (2 f_s) = 7.49 m, the vector of the K range errors by at most sqrt(K)
times that, and the position by at most the largest singular value of the position rows of the pseudo-inverse times that, which is
under pdop (of the five-unknown system, from the restatement): bound = pdop sqrt(K) c / (2 f_s) = 103.7 m here.  The measured value
is printed and stands in DESIGN.md 4.21: 4.1 m, the code phases within 0.12 sample."""
import numpy as np
import pytest

from tests import fix_cases as fc
from tests import snap_cases as sc
from tests import snap_ref as sr
from tests import vel_cases as vc
from tests import vel_ref as vr

pytestmark = pytest.mark.gpu

FC, LC = 1.023e6, 1023.0


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_snapshot_to_velocity_with_nothing_read_back(g):
    c = sc.case("short", 30, 12, 8, check=False)
    moving = vc.moving(c.case)
    iono = g.atmosphere.Klobuchar((1.2e-8, 1.5e-8, -6e-8, -1.2e-7), (9.6e4, 1.3e5, -6.6e4, -5.2e5))
    kw = dict(sigma_m=1.0, init_xyz=tuple(c.prior[0]))
    frac, rx_ms, rx_frac, prior, dop = cuda(c.code_frac), cuda(c.rx_ms), cuda(c.rx_frac), cuda(c.prior), cuda(moving.doppler)
    snap = g.snapshot_fix(c.ephs, frac, rx_ms, rx_frac, prior)
    tx_ms, rx_out = snap.raw("tx_ms"), snap.raw("rx_ms_out")
    fix = g.position_fix_raim(c.ephs, tx_ms, frac, rx_out, rx_frac, **kw)
    atm = g.range_corrections(c.ephs, tx_ms, frac, rx_out, rx_frac, fix, iono=iono, zenith=(2.3, 0.1))
    vel = g.velocity_fix(c.ephs, tx_ms, atm.tx_frac_dev, dop, fix)
    assert all(r._host is None for r in (snap, fix, atm, vel)), "something was read back before the end"

    hs = g.snapshot_fix_host(*c.args())
    hf = g.position_fix_raim_host(c.ephs, hs.tx_ms, c.code_frac, hs.rx_ms_out, c.rx_frac, **kw)
    ha = g.range_corrections_host(c.ephs, hs.tx_ms, c.code_frac, hs.rx_ms_out, c.rx_frac, hf, iono=iono, zenith=(2.3, 0.1))
    hv = g.velocity_fix_host(c.ephs, hs.tx_ms, ha.tx_frac_out, moving.doppler, hf)
    assert snap.fixes.tobytes() == hs.fixes.tobytes() and snap.tx_ms.tobytes() == hs.tx_ms.tobytes()
    assert fix.fixes.tobytes() == hf.fixes.tobytes() and fix.integrity.tobytes() == hf.integrity.tobytes()
    assert atm.tx_frac_out.tobytes() == ha.tx_frac_out.tobytes() and vel.velocities.tobytes() == hv.velocities.tobytes()
    assert (snap.status == 0).all() and (fix.status == 0).all() and (vel.status == 0).all()
    assert np.array_equal(snap.tx_ms, c.case.tx_ms) and np.linalg.norm(fix.xyz - c.truth_xyz, axis=1).max() < 1e-3
    assert np.abs(vel.v_ecef - moving.v_ecef).max() < 1.0  # the corrected fractions carry metres of delay, the velocity stays


def test_acquisition_to_position(g):
    import torch

    fs, N, e = 20.0e6, 20000, 0
    c = sc.case("short", 30, 8, 8, check=False)
    K = c.K
    assert c.seen[e].all() and 6 <= K <= 8
    tau = c.code_frac[e] * FC  # the code phase at the block's first sample: the reception
    doppler = vr.doppler(c.ephs, c.case.tx_ms[e], c.case.tx_frac[e], c.truth_xyz[e], np.zeros(3), 0.0)
    assert np.abs(doppler).max() < 5000.0
    prns = np.arange(K) + 3  # channel k sends the code of table column k + 3
    ctx = g.get_context()
    ctx.set_codes(g.GPSL1().codes)
    prm = g.make_params(prns, FC * (1 + doppler / 1575.42e6), doppler, tau, 0.0, shape=(1, K))
    re = torch.empty((1, N), dtype=torch.float32, device="cuda")
    im = torch.empty_like(re)
    ctx.gen_signal(re, im, g.GAT_LAYOUT_PLANAR, N, 1, N, N, 1, K, ctx.params_to_device(prm), fs, amplitude=1.0,
                   steering_cycles=torch.zeros(1, dtype=torch.float32, device="cuda"), noise_sigma=0.0, seed=1)

    res = g.acquire(g.GPSL1(), (re, im), fs, prns, num_samples=N, max_doppler=5000.0, doppler_step=500.0, code_step_chips=None, method="fft")
    got, frac = g.code_fractions(res, g.GPSL1())
    assert np.array_equal(got, prns) and all(r.detected == 1 for r in res), [(r.prn, r.detected, r.peak_to_second) for r in res]
    off = (frac - c.code_frac[e] + 0.5e-3) % 1e-3 - 0.5e-3
    print("code phase errors in samples:", np.round(off * fs, 3))
    assert np.abs(off).max() <= 0.5 / fs * (1 + 1e-6)

    args = (c.ephs, frac[None, :], c.rx_ms[e:e + 1], c.rx_frac[e:e + 1], c.prior[e:e + 1])
    snap = g.snapshot_fix(c.ephs, *[cuda(a) for a in args[1:]])
    assert snap._host is None
    host = g.snapshot_fix_host(*args)
    assert snap.fixes.tobytes() == host.fixes.tobytes()
    for name in ("tx_ms", "rx_ms_out", "n_ms", "resid", "sin_el", "used"):
        assert getattr(snap, name).tobytes() == getattr(host, name).tobytes(), name

    r = sr.snapshot(c.ephs, c.code_frac[e], c.rx_ms[e], c.rx_frac[e], c.prior[e])
    bound = r["pdop"] * np.sqrt(K) * sr.C / (2 * fs)
    err = float(np.linalg.norm(snap.xyz[0] - c.truth_xyz[e]))
    print(f"acquisition to position: {err:.3f} m off the truth, bound {bound:.3f} m (pdop {r['pdop']:.3f}, K {K}); status {snap.status[0]}, "
          f"rms residual {snap.rms_residual_m[0]:.3f} m, t_c - truth {snap.coarse_time_s[0] - c.offset_ms[e] * 1e-3:.3e} s")
    assert snap.status[0] == 0 and snap.num_used[0] == K and err <= bound
    # t_c carries the ranges' error times tdop (milliseconds): the whole milliseconds handed on are off by the same few in every channel
    shift = snap.tx_ms[0].astype(np.int64) - c.case.tx_ms[e]
    assert (shift == shift[0]).all() and abs(int(shift[0])) <= r["tdop"] * np.sqrt(K) * sr.C / (2 * fs) * 1e3 + 1
    assert snap.rx_ms_out[0] - int(c.case.rx_ms[e]) == shift[0]
