"""CPU forecast of tests/test_spectrum_pipeline_gpu.py, on the library's own conventions and without a device, in the manner of
scripts/filter_forecast.py (whose scene generator, host filter and numpy search it uses): the NOTCH scene of tests/fir_ref.py --
two satellites under a CW tone nobody tells the receiver about --; gat_sample_spectrum_host (the bit-exact twin of the device
spectrum) over the stream as auto_notch cuts it, the float64 mean, find_tones; one notch_taps per tone found through
gat_filter_samples_host; the search on the raw and on the notched stream.  Prints the tones found and, per stream and code-table
column, detected, peak / second, Doppler and code phase.

  python scripts/spectrum_forecast.py [--seed-offset 0]"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from scripts.filter_forecast import host_filter, scene_stream, search  # noqa: E402


def host_mean_spectrum(x, F, H):
    """float64 [M, F]: the stream (complex [M, n], narrowed to float32 as the device holds it) through gat_sample_spectrum_host in
    the blocks spectrum_stream cuts, added in float64 in block order, over the segment count"""
    from gpuacceleratedtracking_amd import spectrum as sp
    from gpuacceleratedtracking_amd.frontend import host_desc
    M, n = x.shape
    re, im = np.ascontiguousarray(x.real.astype(np.float32)), np.ascontiguousarray(x.imag.astype(np.float32))
    S_total, S_block, B, S_rest = sp.stream_partition(n, F, H, M)
    w = sp.window_values("hann", F)
    total = np.zeros((M, F))
    for first, count, seg in ((0, B, S_block), (B * S_block * H, 1 if S_rest else 0, S_rest)):
        if not count:
            continue
        out = np.zeros((count, M, F), np.float32)
        rc = sp.sample_spectrum_host(host_desc(re, im, 0, M, (seg - 1) * H + F, n, seg * H, first), count, w, F, H, out)
        assert rc == 0, rc
        for b in range(count):
            total = total + out[b].astype(np.float64)
    return total / S_total, S_total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed-offset", type=int, default=0)
    ap.add_argument("--num-bins", type=int, default=1024)
    args = ap.parse_args()
    from gpuacceleratedtracking_amd import filtering as f
    from gpuacceleratedtracking_amd import spectrum as sp
    from tests import fir_ref as ref

    s = ref.NOTCH
    x, codes = scene_stream(s, args.seed_offset)
    used = ref.scene_used_samples(s)
    F = args.num_bins
    # the satellites alone: nothing to notch
    psd, S = host_mean_spectrum(x[:, :used], F, F // 2)
    p = psd.sum(axis=0)
    print(f"without the tone: {S} segments, largest bin {10 * np.log10(p.max() / np.median(p)):.2f} dB over the median, tones {sp.find_tones(psd)}", flush=True)
    x = x + ref.scene_tone(s)[None, :]
    psd, S = host_mean_spectrum(x[:, :used], F, F // 2)
    tones = sp.find_tones(psd)
    print(f"with the tone at nu = {s['nu']}: tones {tones}; error {[(t[0] - s['nu']) * F for t in tones]} bins", flush=True)
    search(x[:, :s["out_blocks"] * s["N"]].astype(np.complex64).astype(np.complex128), codes, s["cols"], s["fs"], s["N"], s["out_blocks"], s["max_doppler"], "raw with tone")
    taps = np.ones(1, np.complex128)
    for nu, _ in tones:
        taps = np.convolve(taps, f.notch_taps(s["T"], nu, s["width"]))
    y = host_filter(x[:, :used], taps, 1, 0.0)
    tau, dop = ref.scene_truth(s, (taps.size - 1) / 2.0, s["fs"])
    print(f"blind notch of {taps.size} taps; truth: " + ", ".join(f"column {c}: {d:.0f} Hz {t:.3f} chips" for c, d, t in zip(s["present"], dop, tau)), flush=True)
    search(y, codes, s["cols"], s["fs"], s["N"], s["out_blocks"], s["max_doppler"], "blind notch")


if __name__ == "__main__":
    main()
