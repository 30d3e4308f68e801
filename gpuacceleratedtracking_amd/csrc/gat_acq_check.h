// gat_acq_check.h -- the refusals that both acquisition entry points (through the call check of gat_acq_plan.h), the FFT search's
// plan (gat_acq_fft_plan.h, which is also called bare) and gat_acq_stats_host make about a gat_acq_config, stated once.  No HIP
// call and no HIP header.  (The searches' bound on the code span is the kernels' own predicate, code_span_bad of gat_chan_rules.h,
// which the plans call directly.)
#pragma once

#include <cmath>

#include "gat_chan_rules.h"
#include "gat_sig_plan.h"

namespace gat {

constexpr long long kAcqMaxBins = 1ll << 26; // num_prns * D * J
constexpr int kAcqMaxCodeStep = 31;          // s: the direct search's replica window (kAcqChunk + s * 255 chip pairs) stays within 64 KB of LDS

inline Refusal acq_check_config(const gat_acq_config *cfg, int32_t P, int32_t D, int32_t J, double fs)
{
    if (!cfg) return {GAT_ERR_ARG, "null config"};
    if (cfg->struct_size < sizeof(gat_acq_config)) return {GAT_ERR_ARG, "config.struct_size too small"};
    if (cfg->reserved != 0) return {GAT_ERR_ARG, "config.reserved must be 0"};
    if (P < 1 || D < 1 || J < 1) return {GAT_ERR_ARG, "empty grid (PRNs, Doppler bins and code bins must be positive)"};
    if (D != cfg->num_doppler_bins || J != cfg->num_code_bins) return {GAT_ERR_ARG, "grid size differs from the config"};
    if (cfg->code_step_samples < 1) return {GAT_ERR_ARG, "code step must be at least one sample"};
    if (cfg->code_step_samples > kAcqMaxCodeStep) return {GAT_ERR_RANGE, "code step above 31 samples"};
    if ((long long)P * D * J > kAcqMaxBins) return {GAT_ERR_RANGE, "grid above 2^26 bins"};
    if (!(fs > 0.0) || !std::isfinite(fs)) return {GAT_ERR_ARG, "sampling frequency must be positive"};
    if (!(cfg->code_freq_hz > 0.0) || !std::isfinite(cfg->code_freq_hz)) return {GAT_ERR_ARG, "code frequency must be positive"};
    if (!std::isfinite(cfg->if_hz) || !std::isfinite(cfg->doppler_first_hz) || !std::isfinite(cfg->doppler_step_hz) ||
        !std::isfinite(cfg->min_peak_ratio) || cfg->min_peak_ratio < 0.0)
        return {GAT_ERR_ARG, "bad frequency / threshold"};
    const double fmax = std::fabs(cfg->if_hz) + std::fabs(cfg->doppler_first_hz) + std::fabs(cfg->doppler_step_hz) * (double)D;
    if (!(fmax / fs < 1.0e6)) return {GAT_ERR_RANGE, "carrier frequency out of range"};
    return {GAT_OK, nullptr};
}

} // namespace gat
