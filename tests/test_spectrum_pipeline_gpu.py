"""End-to-end test of the sample spectrum (gpuacceleratedtracking_amd/spectrum.py): a receiver that meets an interferer has to find
it before it can notch it.  The NOTCH scene of tests/fir_ref.py -- two satellites under a CW tone 40 dB over the noise -- is what
tests/test_filter_pipeline_gpu.py notches with the tone's frequency read from the scene; here the receiver is not told:

  * the mean spectrum of the stream shows one tone, within a twentieth of a bin of where it is;
  * the search on the raw stream finds nothing;
  * behind auto_notch the search finds exactly the satellites that are there, where they are.

The scene was fixed with a CPU forecast, scripts/spectrum_forecast.py: the FP64 oracle's generator, numpy noise,
gat_sample_spectrum_host, find_tones, gat_filter_samples_host, a numpy FFT search on the library's grid and gat_acq_stats_host."""
import numpy as np
import pytest

from tests import fir_ref as ref
from tests.fir_ref import FC, LC, NOTCH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


@pytest.fixture(scope="module")
def scene(g):
    """the tone scene on the device: planar (re, im) [M, gen_blocks * N], satellites, noise and the tone"""
    import torch
    s = NOTCH
    prn0, fcode, f, tau, phi = ref.scene_params(s)
    prm = g.make_params(prn0, fcode, f, tau, 2 * np.pi * phi, shape=(s["gen_blocks"], prn0.size))
    re, im = g.gen_signal_stream(g.GPSL1(), prm, s["fs"], s["N"], s["M"], noise_sigma=ref.scene_sigma(s), seed=s["noise_seed"])
    tone = ref.scene_tone(s)
    re = (re + torch.from_numpy(tone.real.astype(np.float32)).to(re.device)[None, :]).contiguous()
    im = (im + torch.from_numpy(tone.imag.astype(np.float32)).to(im.device)[None, :]).contiguous()
    return re, im


def check_found(res, s, delay_out, fs_out):
    """exactly the present columns detected, each within one Doppler bin and one code bin of the truth (the verdicts
    tests/test_filter_pipeline_gpu.py holds its notch to)"""
    assert [r.prn for r in res] == s["cols"]
    assert [r.detected for r in res] == [1 if c in s["present"] else 0 for c in s["cols"]]
    tau, dop = ref.scene_truth(s, delay_out, fs_out)
    N_out = s["N"] // s["D"]
    code_bin = max(1, round(0.5 * fs_out / FC)) * FC / fs_out  # chips
    for c, t, f in zip(s["present"], tau, dop):
        r = res[s["cols"].index(c)]
        assert abs(r.carrier_doppler - f) <= fs_out / (2.0 * N_out)
        assert abs(((r.code_phase - t + LC / 2) % LC) - LC / 2) <= code_bin


def test_the_spectrum_shows_the_tone_nobody_named(g, scene):
    """F = 1024, H = 512, Hann over the 40064 samples the notch will take: 77 segments x 2 antennas.  Forecast
    (scripts/spectrum_forecast.py): one tone at nu = 0.1550000014 (1.5e-6 bin from 0.155), 67.9 dB over the median; without the
    tone the largest bin lies 1.0 dB over the median.  The device draws another noise sequence: the verdict is held, one tone within
    0.05 bin."""
    s = NOTCH
    used = ref.scene_used_samples(s)
    psd, S = g.spectrum_stream(scene, 1024, used)
    assert S == (used - 1024) // 512 + 1 and psd.shape == (s["M"], 1024)
    assert g.get_context().last_launch_info()["vec"] == 4  # an aligned stream with an aligned hop: 16-byte loads
    tones = g.find_tones(psd)
    print("tones:", tones, "error in bins:", [(t[0] - s["nu"]) * 1024 for t in tones])
    assert len(tones) == 1 and abs(tones[0][0] - s["nu"]) * 1024 <= 0.05 and tones[0][1] > 40.0


def test_the_raw_stream_hides_the_satellites_and_auto_notch_uncovers_them(g, scene):
    """Forecast, peak / second of columns 2, 7, 21, 28:
        raw with tone  1.008  1.021  1.017  1.004  -> nothing detected
        blind notch    4.913  1.015  5.065  1.169  -> exactly the two present ones, at -2162.4 Hz / 89.223 chips and 3952.3 Hz /
                                                      513.881 chips against the truth -2250 / 89.237 and 3900 / 513.837
    -- the ratios of the notch that is told the tone (tests/test_filter_pipeline_gpu.py): the estimate is 1.5e-6 bin off, the
    notch 0.01 cycles per sample wide.  One tone: 65 taps, a delay of 32 samples = 1.637 chips.  The device draws another noise
    sequence: the verdicts are held, not the ratios."""
    s = NOTCH
    system, N, B = g.GPSL1(), s["N"], s["out_blocks"]
    raw = g.acquire(system, scene, s["fs"], s["cols"], num_samples=N, num_blocks=B, max_doppler=s["max_doppler"])
    print("raw:", [(r.prn, r.detected, round(r.peak_to_second, 3)) for r in raw])
    assert all(r.detected == 0 for r in raw)
    (yr, yi), desc, tones = g.auto_notch(scene, ref.scene_used_samples(s))
    assert len(tones) == 1 and abs(tones[0][0] - s["nu"]) * 1024 <= 0.05
    assert desc.num_samples == B * N and desc.num_ants == s["M"]
    res = g.acquire(system, (yr, yi), s["fs"], s["cols"], num_samples=N, num_blocks=B, max_doppler=s["max_doppler"])
    print("blind notch:", [(r.prn, r.detected, round(r.peak_to_second, 3), round(r.carrier_doppler, 1), round(r.code_phase, 3)) for r in res])
    check_found(res, s, (s["T"] - 1) / 2.0, s["fs"])
