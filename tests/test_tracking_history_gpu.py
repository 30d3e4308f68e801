"""gat_tracking_run_history (TrackingLoop.run_history): the native run that keeps the parameters every block was correlated with.
Three PRNs, 1 and 4 antennas, N = 2046, 1, 2 and 25 blocks, with and without beamformer weights: accumulators, loop state and
current parameters are byte-identical to ``run`` from the same start, record 0 is the start and the last record the current
parameters, and every record b + 1 is what gat_tracking_update_host makes of block b's accumulators and record b, within the
tolerance test_tracking_loop_gpu.py holds the device update to against the host's equations (rtol 1e-12, atol 1e-9).
GAT_FLAG_GRAPH is refused."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, FS, NBLK = 2046, 2.046e6, 25
PRNS = np.array([4, 12, 29])
DOP = np.array([900.0, -1750.0, 60.0])
TAU0 = np.array([33.25, 512.5, 1001.75])


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@functools.lru_cache(maxsize=None)
def signal(M):
    import gpuacceleratedtracking_amd as g

    system = g.GPSL1()
    fcode = 1.023e6 * (1 + DOP / 1575.42e6)
    b = np.arange(NBLK, dtype=np.float64)[:, None]
    tau = np.mod(TAU0[None, :] + fcode[None, :] * (N / FS) * b, 1023.0)
    phi = np.mod(DOP[None, :] * (N / FS) * b, 1.0)
    prm = g.make_params(PRNS - 1, fcode, DOP, tau, 2 * np.pi * phi, shape=(NBLK, 3))
    re, im = g.gen_signal_stream(system, prm, FS, N, M)
    shifts = g.get_correlator_sample_shifts(system, g.EarlyPromptLateCorrelator(M, 3), FS, 0.5)
    return system, re, im, shifts


def make(g, M, weights):
    system, re, im, shifts = signal(M)
    w = None
    if weights:
        rng = np.random.default_rng(M)
        w = (1.0 + 0.2 * rng.standard_normal((3, M)) + 0.2j * rng.standard_normal((3, M))) / M
    return g.TrackingLoop(system, PRNS, N, M, FS, shifts, init_carrier_doppler=DOP + 4.0, init_code_phase=TAU0 + 0.05, dll_bandwidth_hz=4.0,
                          weights=w), w


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("nb", [1, 2, 25])
@pytest.mark.parametrize("M", [1, 4])
def test_history_run_equals_run(g, M, nb, weights):
    from gpuacceleratedtracking_amd import _lib

    _, re, im, _ = signal(M)
    a, _ = make(g, M, weights)
    b, w = make(g, M, weights)
    start, state0 = b.params().reshape(-1).copy(), b.state().copy()
    acc_re, acc_im = a.run(re, im, nb)
    h_re, h_im, history = b.run_history(re, im, nb)
    assert tuple(history.shape) == (nb + 1, 3, 40) and b.blocks_done == nb
    assert h_re.cpu().numpy().tobytes() == acc_re.cpu().numpy().tobytes() and h_im.cpu().numpy().tobytes() == acc_im.cpu().numpy().tobytes()
    assert a.state().tobytes() == b.state().tobytes() and a.params().tobytes() == b.params().tobytes()
    assert a.accumulators().tobytes() == b.accumulators().tobytes()
    rec = history.cpu().numpy().view(_lib.PARAMS_DTYPE).reshape(nb + 1, 3)
    assert rec[0].tobytes() == start.tobytes() and rec[nb].tobytes() == b.params().reshape(-1).tobytes()
    # every record from its predecessor by the host's update
    lib, state = _lib.load(), state0.copy()
    re_h, im_h = h_re.cpu().numpy(), h_im.cpu().numpy()
    w_re = None if w is None else np.ascontiguousarray(w.real, np.float64)
    w_im = None if w is None else np.ascontiguousarray(w.imag, np.float64)
    for blk in range(nb):
        cur, nxt = np.ascontiguousarray(rec[blk]), np.zeros(3, _lib.PARAMS_DTYPE)
        args = (C.c_void_p(re_h[blk].ctypes.data), C.c_void_p(im_h[blk].ctypes.data), 3, M, C.byref(b.config), C.c_void_p(state.ctypes.data),
                C.c_void_p(cur.ctypes.data), C.c_void_p(nxt.ctypes.data))
        rc = lib.gat_tracking_update_host(*args) if w is None else lib.gat_tracking_update_host_weighted(*args, C.c_void_p(w_re.ctypes.data),
                                                                                                        C.c_void_p(w_im.ctypes.data))
        assert rc == 0
        assert (nxt["prn"] == rec[blk + 1]["prn"]).all()
        for f in ("code_freq_hz", "carrier_freq_hz", "code_phase_chips", "carrier_phase_cycles"):
            assert np.allclose(rec[blk + 1][f], nxt[f], rtol=1e-12, atol=1e-9), (blk, f, rec[blk + 1][f], nxt[f])
    # a second call continues from record nb, as run does
    if nb == 2:
        a.run(re, im, nb, start=nb * N)
        _, _, more = b.run_history(re, im, nb, start=nb * N)
        assert a.params().tobytes() == b.params().tobytes() and a.state().tobytes() == b.state().tobytes()
        assert more[0].cpu().numpy().tobytes() == history[nb].cpu().numpy().tobytes()


def test_history_run_refuses_a_graph(g):
    import torch
    from gpuacceleratedtracking_amd import _lib
    from gpuacceleratedtracking_amd.streams import input_desc

    _, re, im, _ = signal(1)
    loop, _ = make(g, 1, False)
    before = loop.params().tobytes()
    _, desc = input_desc((re, im), N, 2, 0)
    acc = torch.zeros((2, 3, 3, 1), dtype=torch.float32, device=loop.ctx.device)
    acc_im = torch.zeros_like(acc)
    hist = torch.zeros((3, 3, 40), dtype=torch.uint8, device=loop.ctx.device)

    def call(flags, w_re=None, w_im=None, history=hist):
        return loop.ctx.lib.gat_tracking_run_history(loop.ctx._h, C.byref(desc), 2, 3, 3, loop.shifts.ctypes.data_as(C.POINTER(C.c_int32)), FS,
                                                     C.byref(loop.config), C.c_void_p(loop._state.data_ptr()),
                                                     None if history is None else C.c_void_p(history.data_ptr()), C.c_void_p(acc.data_ptr()),
                                                     C.c_void_p(acc_im.data_ptr()), 9, flags, w_re, w_im)
    assert call(_lib.GAT_FLAG_GRAPH) == 1
    assert call(_lib.GAT_FLAG_GRAPH | _lib.GAT_FLAG_ATOMIC) == 1
    assert call(0, history=None) == 1
    assert call(0, w_re=C.c_void_p(acc.data_ptr())) == 1  # one weight pointer without the other
    loop.ctx.sync()
    assert not hist.any() and not acc.any() and loop.params().tobytes() == before
