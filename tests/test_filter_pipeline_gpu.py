"""End-to-end tests of the sample filter (gpuacceleratedtracking_amd/filtering.py): what changing a stream's band and rate is for.

  * a wideband front end -- 100 MHz, the band on a 12.5 MHz IF -- is channelised to 20 MHz baseband and the search at 20 MHz finds
    exactly the satellites that are there, where they are;
  * a CW tone hides the satellites from the search on the raw stream; behind a notch the search finds them;
  * the filtered stream goes on through the conditioner to int8 and still acquires.

The scenes (tests/fir_ref.py CHANNEL, NOTCH) were fixed with a CPU forecast, scripts/filter_forecast.py: the FP64 oracle's
generator, numpy noise, gat_filter_samples_host, a numpy FFT search on the library's grid and gat_acq_stats_host."""
import numpy as np
import pytest

from tests import fir_ref as ref
from tests.fir_ref import CHANNEL, FC, LC, NOTCH

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def g():
    import gpuacceleratedtracking_amd as g
    g.load_library()
    return g


def scene_stream(g, s):
    """the scene's satellites and noise on the device: planar (re, im) [M, gen_blocks * N]"""
    prn0, fcode, f, tau, phi = ref.scene_params(s)
    prm = g.make_params(prn0, fcode, f, tau, 2 * np.pi * phi, shape=(s["gen_blocks"], prn0.size))
    return g.gen_signal_stream(g.GPSL1(), prm, s["fs"], s["N"], s["M"], noise_sigma=ref.scene_sigma(s), seed=s["noise_seed"])


def check_found(res, s, delay_out, fs_out):
    """exactly the present columns detected, each within one Doppler bin and one code bin of the truth"""
    assert [r.prn for r in res] == s["cols"]
    assert [r.detected for r in res] == [1 if c in s["present"] else 0 for c in s["cols"]]
    tau, dop = ref.scene_truth(s, delay_out, fs_out)
    N_out = s["N"] // s["D"]
    code_bin = max(1, round(0.5 * fs_out / FC)) * FC / fs_out  # chips
    for c, t, f in zip(s["present"], tau, dop):
        r = res[s["cols"].index(c)]
        assert abs(r.carrier_doppler - f) <= fs_out / (2.0 * N_out)
        assert abs(((r.code_phase - t + LC / 2) % LC) - LC / 2) <= code_bin


def test_channelise_a_wideband_stream_and_acquire(g):
    """Three satellites of 45 dB-Hz (amplitude 1 in noise of sigma = 39.76 per component at 100 MHz) on a 12.5 MHz IF, 2 antennas;
    channelize(cutoff 5 MHz, decimation 5, 64 taps) gives 2 x 1 ms at 20 MHz baseband, searched for 6 columns over +-5 kHz.
    Forecast (scripts/filter_forecast.py), peak / second of columns 4, 9, 12, 17, 25, 30:
        4.687  1.056  4.791  1.008  6.387  1.071  -> exactly the three present ones (threshold 2.0), at 1816.1 Hz / 211.761 chips,
        -3045.7 Hz / 641.000 chips and 413.5 Hz / 999.462 chips against the truth 1800 / 211.622, -3100 / 641.072, 400 / 999.422
    (another noise seed: 4.244, 6.249, 6.642).  The reported group delay is 6.3 output samples = 0.322 chips; a Doppler bin is
    500 Hz, a code bin 10 samples = 0.5115 chips.  The device draws another noise sequence: the verdicts are held, not the ratios."""
    s = CHANNEL
    re, im = scene_stream(g, s)
    used = ref.scene_used_samples(s)
    (yr, yi), desc, fs_out, delay = g.channelize((re, im), s["fs"], s["if_hz"], s["cutoff_hz"], s["D"], s["T"], total_samples=used)
    N_out = s["N"] // s["D"]
    assert fs_out == 20e6 and delay == 6.3 and desc.num_samples == s["out_blocks"] * N_out and desc.num_ants == s["M"]
    assert g.get_context().last_launch_info()["vec"] > 1  # an aligned stream: the tiled kernel
    res = g.acquire(g.GPSL1(), (yr, yi), fs_out, s["cols"], num_samples=N_out, num_blocks=s["out_blocks"], max_doppler=s["max_doppler"])
    print("channelised:", [(r.prn, r.detected, round(r.peak_to_second, 3), round(r.carrier_doppler, 1), round(r.code_phase, 3)) for r in res])
    check_found(res, s, delay, fs_out)


@pytest.fixture(scope="module")
def notched(g):
    """the tone scene on the device, raw and behind the notch"""
    import torch
    s = NOTCH
    re, im = scene_stream(g, s)
    tone = ref.scene_tone(s)
    re = (re + torch.from_numpy(tone.real.astype(np.float32)).to(re.device)[None, :]).contiguous()
    im = (im + torch.from_numpy(tone.imag.astype(np.float32)).to(im.device)[None, :]).contiguous()
    taps = g.notch_taps(s["T"], s["nu"], s["width"])
    (yr, yi), desc = g.filter_stream((re, im), taps, ref.scene_used_samples(s))
    return dict(re=re, im=im, yr=yr, yi=yi, desc=desc)


def test_a_notch_uncovers_the_satellites_under_a_cw_tone(g, notched):
    """Two satellites of 47 dB-Hz (sigma = 14.13 at 20 MHz), 2 antennas, 2 x 1 ms, and a CW tone 40 dB over the noise power in
    20 MHz (amplitude 1997.6) 3.1 MHz off the carrier; notch_taps(65, 0.155, 0.01).  Forecast, peak / second of columns 2, 7, 21, 28:
        raw with tone  1.008  1.021  1.017  1.004  -> nothing detected
        notched        4.913  1.015  5.065  1.169  -> exactly the two present ones, at -2162.4 Hz / 89.223 chips and 3952.3 Hz /
                                                      513.881 chips against the truth -2250 / 89.237 and 3900 / 513.837
    (another noise seed: 6.171 and 3.174).  The notch delays the stream by 32 samples = 1.637 chips."""
    s = NOTCH
    system, N, B = g.GPSL1(), s["N"], s["out_blocks"]
    raw = g.acquire(system, (notched["re"], notched["im"]), s["fs"], s["cols"], num_samples=N, num_blocks=B, max_doppler=s["max_doppler"])
    print("raw:", [(r.prn, r.detected, round(r.peak_to_second, 3)) for r in raw])
    assert all(r.detected == 0 for r in raw if r.prn in s["present"])
    assert notched["desc"].num_samples == B * N
    res = g.acquire(system, (notched["yr"], notched["yi"]), s["fs"], s["cols"], num_samples=N, num_blocks=B, max_doppler=s["max_doppler"])
    print("notched:", [(r.prn, r.detected, round(r.peak_to_second, 3), round(r.carrier_doppler, 1), round(r.code_phase, 3)) for r in res])
    check_found(res, s, (s["T"] - 1) / 2.0, s["fs"])


def test_the_filtered_stream_goes_on_through_the_conditioner(g, notched):
    """filter_samples' output through requantize to int8 (forecast: 4.918 and 5.044, nothing lost) into the search, by descriptor"""
    import torch
    s = NOTCH
    N, B = s["N"], s["out_blocks"]
    sig8, desc, counts, params = g.requantize((notched["yr"], notched["yi"]), N, B)
    assert sig8.dtype == torch.int8 and desc.num_samples == N and int(counts.cpu().numpy()[:, 1].sum()) == 0
    res = g.acquire(g.GPSL1(), desc, s["fs"], s["cols"], num_blocks=B, max_doppler=s["max_doppler"])
    print("notched int8:", [(r.prn, r.detected, round(r.peak_to_second, 3)) for r in res])
    check_found(res, s, (s["T"] - 1) / 2.0, s["fs"])
