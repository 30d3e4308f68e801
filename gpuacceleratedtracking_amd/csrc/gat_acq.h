// gat_acq.h -- the acquisition search's per-PRN statistics (peak, noise set, parabola refinement, C/N0, detection), written
// once for the device kernel (acq_stats_kernel, gat_acq.hip) and for the host entry point gat_acq_stats_host
// (gat_acq_api.cpp).  Double precision; compiled without contraction in both builds.
#pragma once

#include <math.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

constexpr double kAcqExclusionChips = 1.5; // the noise set: circular code distance from the peak beyond this
constexpr long long kAcqMinNoiseBins = 64; // fewer noise bins: no noise estimate (NaN, detected = -1)
constexpr double kAcqDefaultPeakRatio = 2.0;

// code phase (chips, in [0, Lc)) of the (fractional) code bin j at sample 0 of block 0
GAT_HD inline double acq_code_phase(const gat_acq_config &c, double fs, double j)
{
    const double Lc = (double)c.code_length;
    double ph = c.code_freq_hz / fs * ((double)c.first_shift + (double)c.code_step_samples * j);
    ph -= floor(ph / Lc) * Lc;
    return (ph >= Lc || ph < 0.0) ? 0.0 : ph;
}

// is code bin j (phase ph) in the noise set of a peak at phase ph_peak
GAT_HD inline bool acq_in_noise_set(double ph, double ph_peak, double Lc)
{
    double d = fabs(ph - ph_peak);
    d = d < Lc - d ? d : Lc - d;
    return d > kAcqExclusionChips;
}

// vertex offset of the parabola through (-1, a), (0, b), (1, c), clamped to +-0.5; 0 when it is not a maximum
GAT_HD inline double acq_parabola(double a, double b, double c)
{
    const double den = a - 2.0 * b + c;
    if (!(den < 0.0)) return 0.0;
    double d = 0.5 * (a - c) / den;
    if (!(d == d)) return 0.0;
    return d > 0.5 ? 0.5 : (d < -0.5 ? -0.5 : d);
}

// Everything but the reductions: the peak (i, j) and its power, the powers of its four neighbours (NaN where the grid ends),
// the noise set's sum, size and maximum.  N: samples per block (the C/N0's coherent time N / fs).
GAT_HD inline void acq_finish(const gat_acq_config &c, double fs, long long N, int D, int J, int i, int j, double peak,
                              double left_d, double right_d, double left_j, double right_j, double noise_sum,
                              long long noise_count, double second, gat_acq_result &r)
{
    const double ratio_min = c.min_peak_ratio > 0.0 ? c.min_peak_ratio : kAcqDefaultPeakRatio;
    const double di = (i > 0 && i < D - 1) ? acq_parabola(left_d, peak, right_d) : 0.0;
    const double dj = (j > 0 && j < J - 1) ? acq_parabola(left_j, peak, right_j) : 0.0;
    r.doppler_bin = i;
    r.code_bin = j;
    r.peak_power = peak;
    r.carrier_doppler_hz = c.doppler_first_hz + ((double)i + di) * c.doppler_step_hz;
    r.code_phase_chips = acq_code_phase(c, fs, (double)j + dj);
    r.num_noise_bins = noise_count;
    if (noise_count < kAcqMinNoiseBins) {
        const double nan = __builtin_nan("");
        r.noise_power = r.second_power = r.peak_to_second = r.cn0_dbhz = nan;
        r.detected = -1;
        return;
    }
    const double noise = noise_sum / (double)noise_count;
    r.noise_power = noise;
    r.second_power = second;
    r.peak_to_second = peak / second;
    r.cn0_dbhz = 10.0 * log10((peak - noise) / (noise * ((double)N / fs)));
    r.detected = r.peak_to_second >= ratio_min ? 1 : 0;
}

} // namespace gat
