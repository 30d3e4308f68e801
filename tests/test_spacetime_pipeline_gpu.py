"""Space-time adaptive processing end to end on the device: spacetime_covariance -> spacetime_weights -> spacetime_filter ->
acquire on the scene of tests/st_ref.py (two antennas, two CW jammers 40 dB over the noise from two directions, one satellite
22 dB under it; tests/test_spacetime_host.py holds the same verdicts in FP64 and with the host twin, with the measured ratios)."""
import numpy as np
import pytest

from tests import st_ref as ref

pytestmark = pytest.mark.gpu


def test_the_jammed_scene_end_to_end():
    """Not detected behind spatial power inversion, detected behind five taps an antenna (power inversion referenced to tap 2,
    antenna 0, no loading) at the true code phase once corrected by spacetime_delay, output power within 3 dB of the noise.
    The device weights against gat_array_weights_host on the FP64 covariance (narrowed to the float32 the solver reads), max |w_dev -
    w_ref| / max |w_ref|: 1e-6 is out of reach of ANY float32 covariance here -- the matrix has a condition number of 1.2e5, and
    already the FP64 covariance rounded to float32 moves the FP64 weights by 3.1e-4, numpy's complex64 sums (in runs of 256 or as one
    product) by 2.2e-3 and 2.8e-3.  Measured on the device: 1.092e-3 (its two-level sums are closer than numpy's); the test holds
    it to a factor 4 over that, 4.4e-3, and prints the value.  Measured verdicts: peak / second 1.05 behind the spatial weights at
    37.1 dB over the noise, 7.12 behind the five-tap ones at 1.18 dB, code phase 417.398 chips for a truth of 417.402."""
    import torch

    import gpuacceleratedtracking_amd as g
    s = ref.SCENE
    N, T, M, col = s["N"], s["T"], s["M"], s["col"]
    n_tot = N + T - 1
    x, _ = ref.scene_stream(s)
    ctx = g.get_context()
    sig = tuple(torch.from_numpy(np.ascontiguousarray(p.astype(np.float32))).to(ctx.device) for p in (x.real, x.imag))
    system = g.GPSL1()
    noise = 2.0 * ref.scene_sigma(s) ** 2

    # the array alone: one degree of freedom against two jammers
    R1 = g.spacetime_covariance(sig, n_tot, num_taps=1)[0]
    w1 = g.spacetime_weights(R1, M, 1)
    (y1r, y1i), d1 = g.spacetime_filter(sig, w1, 1, N)
    r1 = g.acquire(system, d1, s["fs"], [col], max_doppler=s["max_doppler"])[0]
    p1 = 10 * np.log10(float((y1r.double() ** 2 + y1i.double() ** 2).mean()) / noise)

    # five taps an antenna
    R5 = g.spacetime_covariance(sig, n_tot, num_taps=T)[0]
    w5 = g.spacetime_weights(R5, M, T, ref_tap=s["ref_tap"])
    (y5r, y5i), d5 = g.spacetime_filter(sig, w5, T, n_tot)
    assert d5.num_samples == N
    r5 = g.acquire(system, d5, s["fs"], [col], max_doppler=s["max_doppler"])[0]
    p5 = 10 * np.log10(float((y5r[:, :N].double() ** 2 + y5i[:, :N].double() ** 2).mean()) / noise)
    d = g.spacetime_delay(T, s["ref_tap"])
    truth = ref.scene_truth(s, d)
    err = (r5.code_phase - truth + ref.LC / 2) % ref.LC - ref.LC / 2
    print(f"spatial: detected {r1.detected} peak/second {r1.peak_to_second:.2f} at {p1:.1f} dB; five taps: detected {r5.detected} "
          f"peak/second {r5.peak_to_second:.2f} at {p5:.2f} dB, code phase {r5.code_phase:.3f} (truth {truth:.3f}), Doppler {r5.carrier_doppler:.0f} Hz")
    assert r1.detected == 0
    assert r5.detected == 1
    assert abs(err) <= 0.5 * ref.FC / s["fs"]
    assert abs(r5.carrier_doppler - s["dop"]) <= s["fs"] / (2.0 * N)
    assert abs(p5) <= 3.0

    # the device weights against the host solver on the FP64 covariance
    R64 = ref.covariance(x.real.astype(np.float32).astype(np.float64) + 1j * x.imag.astype(np.float32).astype(np.float64), n_tot, 1, T, 1)[0]
    a = ref.steering([1, 0], T, s["ref_tap"])
    Q = M * T
    c_re, c_im = np.ascontiguousarray(R64.real.astype(np.float32)), np.ascontiguousarray(R64.imag.astype(np.float32))
    a_re, a_im = np.ascontiguousarray(a.real), np.ascontiguousarray(a.imag)
    w_re, w_im = np.zeros(Q), np.zeros(Q)
    assert g.load_library().gat_array_weights_host(c_re.ctypes.data, c_im.ctypes.data, Q, a_re.ctypes.data, a_im.ctypes.data, 1, 1, 0.0,
                                                   w_re.ctypes.data, w_im.ctypes.data) == 0
    w_ref = w_re + 1j * w_im
    rel = np.abs(w5.cpu().numpy()[0] - w_ref).max() / np.abs(w_ref).max()
    print(f"device weights against the host solver on the FP64 covariance: {rel:.3e} relative")
    assert rel <= 4.4e-3
