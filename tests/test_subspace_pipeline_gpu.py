"""Self-calibration of an uncalibrated array end to end (the scene and its CPU restatement: tests/sub_pipeline.py).

(a) bootstrap: ``TrackingLoop(weights = e0 rows)`` tracks both satellites on antenna 0 alone, 40 blocks settle, then blocks are kept;
    ``loop.steering`` over the first 400 kept blocks gives a^ per channel from the accumulators where the loop left them.  The miss
    1 - |a^H a^|^2 / (M |a^|^2) stays below 8 (M - 1) / (M B SNR) (1 + 1 / (M SNR)) = 4.84e-4 with B = 400 and SNR = N / (2 sigma^2)
    = 31.25: eight times the first-order miss of a principal eigenvector from B snapshots.  The FP64 restatement over 20 noise
    seeds x 2 channels gave a mean of 6.56e-5 and a largest of 1.75e-4.
(b) a second loop on ``beamformer_weights(None, a^, "conventional")`` over the same stream: the monitor's C/N0 over the 800 kept
    blocks, both estimators, exceeds the antenna-0 loop's by 10 log10 M = 6.02 dB.  The margin was fixed beforehand on the CPU from
    the restatement (oracle.np_correlate, array_ref.tracking_update_weighted, tests/mon_ref.py; ``python -m tests.sub_pipeline``) over
    20 seeds x 2 channels: the gain minus 6.02 dB was -0.197 dB in the mean with a standard deviation of 0.213 dB (-0.657 .. +0.256) for the
    narrow-to-wide estimator and -0.255 dB with 0.283 dB (-0.855 .. +0.245) for the moments estimator; the test allows the mean -+ three
    standard deviations, 0.64 dB and 0.85 dB (tests/sub_pipeline.py GAIN_EXPECTED), under 1 dB for both.
    Over 400 kept blocks the moments estimator's three standard deviations were 1.07 dB, so the run was lengthened to 800.  The
    mean is below zero because the other satellite's cross-correlation is beamformed with the same gain as the signal: it is
    noise the array does not average down.
(c) the source count: the eigenvalues of ``spatial_covariance`` of the jammer scene of tests/test_array_gpu.py say one source for
    its interference (unit noise plus the 40 dB jammer) and none for the noise alone; with that scene's satellite in, which is
    12 dB over the noise per antenna before correlation, they say two and one."""
import numpy as np
import pytest

from tests import sub_pipeline as sp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture(scope="module")
def scene(g):
    system = g.GPSL1()
    fcode, tau, phi, _ = sp.truth()
    prm = g.make_params(sp.PRNS - 1, fcode, sp.DOP, tau, 2 * np.pi * phi, shape=(sp.BLOCKS, sp.PRNS.size))
    re, im = g.gen_signal_stream(system, prm, sp.FS, sp.N, sp.M, steering_cycles=sp.STEER, noise_sigma=sp.SIGMA, seed=2025)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(sp.M, 3), sp.FS, 0.5)

    def loop(weights):
        return g.TrackingLoop(system, sp.PRNS, sp.N, sp.M, sp.FS, shifts, init_carrier_doppler=sp.DOP + 0.2, init_code_phase=sp.TAU0 + 0.02,
                              init_carrier_phase=np.mod(sp.PHI0 + 0.02, 1.0), dll_bandwidth_hz=4.0, weights=weights)
    return re, im, loop


def test_bootstrap_steering_and_beamformed_loop(g, scene):
    re, im, make_loop = scene
    K, M = sp.PRNS.size, sp.M
    e0 = np.zeros((K, M), np.complex128)
    e0[:, 0] = 1.0
    # (a)
    first = make_loop(e0)
    acc_re, acc_im = first.run(re, im, sp.BLOCKS, keep=True)
    kept = slice(sp.SETTLE, sp.SETTLE + sp.ESTIMATE)
    steer, lam = first.steering(acc_re[kept], acc_im[kept])
    first.ctx.sync()
    a_hat = steer.cpu().numpy()
    assert a_hat.shape == (1, K, M) and tuple(lam.shape) == (1, K, M)
    missed = sp.miss(a_hat[0])
    print("miss", missed, "bound", sp.steering_bound(), "eigenvalues", lam.cpu().numpy()[0])
    assert (missed <= sp.steering_bound()).all(), missed
    assert (a_hat[0, :, 0].real > 0).all() and np.abs(a_hat[0, :, 0].imag).max() <= 1e-15
    # the plain antenna sum of this array would have lost the signal: |sum_m a_m|^2 = 0.092 of 16
    assert abs(np.abs(np.exp(2j * np.pi * sp.STEER).sum()) ** 2 - 0.092) < 1e-3
    # (b)
    w = g.beamformer_weights(None, steer[0], "conventional")
    second = make_loop(w)
    bre, bim = second.run(re, im, sp.BLOCKS, keep=True)
    B = sp.KEPT
    mons = []
    for loop, (r, i) in ((first, (acc_re, acc_im)), (second, (bre, bim))):
        mons.append(loop.monitor(r[sp.SETTLE:], i[sp.SETTLE:], first_block=sp.SETTLE, window_blocks=B))
    first.ctx.sync()
    m0, m1 = mons
    assert m0.synced.all() and m1.synced.all() and list(m0.symbol_offset) == [0, 0] and list(m1.symbol_offset) == [0, 0]
    assert (m0.phase_lock > 0.8).all() and (m1.phase_lock > 0.9).all()
    gain = {"nwpr": m1.cn0_nwpr - m0.cn0_nwpr - sp.GAIN_DB, "m2m4": m1.cn0_m2m4[:, 0] - m0.cn0_m2m4[:, 0] - sp.GAIN_DB}
    print("antenna 0: nwpr", m0.cn0_nwpr, "m2m4", m0.cn0_m2m4[:, 0], "beam: nwpr", m1.cn0_nwpr, "m2m4", m1.cn0_m2m4[:, 0], "gain - 6.02 dB", gain)
    for name, (mean, margin) in sp.GAIN_EXPECTED.items():
        assert margin <= 1.0
        assert (np.abs(gain[name] - mean) <= margin).all(), (name, gain[name], mean, margin)
    # the bits of both loops are the scene's, up to the Costas loop's sign
    nsym = B // 20
    for mon in mons:
        for k in range(K):
            sent, got = sp.BITS[k][sp.SETTLE // 20:sp.SETTLE // 20 + nsym], mon.bits[k, :nsym]
            assert np.array_equal(got, sent) or np.array_equal(got, -sent), k


def test_source_count_of_the_jammer_scene(g):
    import torch
    from tests import test_array_gpu as tag
    nblk, N = 8, tag.SCENE["N"]
    snapshots = nblk * N
    ctx = g.get_context()

    def count(x_re, x_im):
        cov = g.spatial_covariance((x_re.contiguous(), x_im.contiguous()), N, nblk)
        lam, _, status = g.hermitian_eig(cov, 0)
        ctx.sync()
        assert int(status[0]) >= 0
        return g.source_count(lam[0], snapshots, "mdl"), g.source_count(lam[0], snapshots, "aic"), lam[0].cpu().numpy()

    re, im, x_in, _ = tag.scene_signal(g, nblk)
    dev = re.device
    jam = x_in.to(dev)
    gen = torch.Generator().manual_seed(tag.SCENE["seed"])  # the scene's noise draws (scene_interference) without its jammer
    quiet = torch.view_as_complex(torch.randn((tag.SCENE["M"], nblk * N, 2), generator=gen, dtype=torch.float32) * (0.5 ** 0.5)).to(dev)
    with_jammer = count(jam.real, jam.imag)
    noise_alone = count(quiet.real, quiet.imag)
    whole = count(re, im)
    whole_quiet = count(re - jam.real + quiet.real, im - jam.imag + quiet.imag)
    print("interference", with_jammer, "noise", noise_alone, "scene", whole, "scene without the jammer", whole_quiet)
    assert with_jammer[0] == 1 and noise_alone[0] == 0  # (the default criterion, MDL; AIC is printed)
    assert whole[0] == 2 and whole_quiet[0] == 1
