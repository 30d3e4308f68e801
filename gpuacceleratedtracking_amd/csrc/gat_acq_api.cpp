// gat_acq_api.cpp -- host side of the acquisition search (include/gat.h gat_acquire, gat_acq_stats_host): validation, the
// grid's work split, the launch sequence {grid, group sum, statistics}, and the statistics on the host (csrc/gat_acq.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "gat_acq.h"
#include "gat_acq_check.h"
#include "gat_acq_kernels.h"
#include "gat_ctx.h"

using namespace gat;

namespace {

constexpr size_t kMaxGroupScratch = (size_t)1 << 30; // bytes of the groups' slices

// the configuration's refusals (gat_acq_check.h, shared with gat_acquire_fft), reported on the context
int32_t check_config(gat_ctx *c, const gat_acq_config *cfg, int32_t P, int32_t D, int32_t J, double fs)
{
    const Refusal r = acq_check_config(cfg, P, D, J, fs);
    return r.code == GAT_OK ? GAT_OK : fail(c, r.code, r.msg);
}

void stats_host(const float *power, int32_t P, int32_t D, int32_t J, const gat_acq_config &cfg, double fs, long long N,
                gat_acq_result *res)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const long long cells = (long long)D * J;
    std::vector<double> phase(J);
    for (int j = 0; j < J; ++j) phase[j] = acq_code_phase(cfg, fs, (double)j);
    for (int p = 0; p < P; ++p) {
        const float *g = power + (size_t)p * cells;
        long long pk = 0;
        float best = -1.0f;
        for (long long c = 0; c < cells; ++c)
            if (g[c] > best) best = g[c], pk = c;
        const int pi = (int)(pk / J), pj = (int)(pk % J);
        double sum = 0.0, second = -1.0;
        long long cnt = 0;
        for (int i = 0; i < D; ++i)
            for (int j = 0; j < J; ++j)
                if (acq_in_noise_set(phase[j], phase[pj], (double)cfg.code_length)) {
                    const float v = g[(size_t)i * J + j];
                    sum += (double)v;
                    ++cnt;
                    second = std::max(second, (double)v);
                }
        gat_acq_result r{};
        r.prn = p;
        acq_finish(cfg, fs, N, D, J, pi, pj, (double)g[pk], pi > 0 ? (double)g[pk - J] : nan, pi < D - 1 ? (double)g[pk + J] : nan,
                   pj > 0 ? (double)g[pk - 1] : nan, pj < J - 1 ? (double)g[pk + 1] : nan, sum, cnt, second, r);
        res[p] = r;
    }
}

} // namespace

GAT_API int32_t gat_acq_stats_host(const float *power, int32_t P, int32_t D, int32_t J, const gat_acq_config *cfg, double fs,
                                   int64_t N, gat_acq_result *res)
{
    if (!power || !res) return GAT_ERR_ARG;
    const int32_t rc = check_config(nullptr, cfg, P, D, J, fs);
    if (rc != GAT_OK) return rc;
    if (cfg->code_length < 1) return GAT_ERR_ARG;
    if (N < 1) return GAT_ERR_ARG;
    stats_host(power, P, D, J, *cfg, fs, (long long)N, res);
    return GAT_OK;
}

GAT_API int32_t gat_acquire(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const int32_t *prns, int32_t P, double fs,
                            const gat_acq_config *cfg_in, float *power_dev, gat_acq_result *res)
{
    if (!c) return GAT_ERR_ARG;
    if (!sig || !prns || !res) return fail(c, GAT_ERR_ARG, "null argument");
    if (!c->d_codes) return fail(c, GAT_ERR_STATE, "gat_set_codes has not been called");
    if (!cfg_in) return fail(c, GAT_ERR_ARG, "null config");
    {
        const int32_t rc = check_config(c, cfg_in, P, cfg_in->num_doppler_bins, cfg_in->num_code_bins, fs);
        if (rc != GAT_OK) return rc;
    }
    gat_acq_config cfg = *cfg_in;
    cfg.struct_size = sizeof(gat_acq_config);
    if (cfg.code_length == 0) cfg.code_length = c->Lc;
    if (cfg.code_length != c->Lc) return fail(c, GAT_ERR_ARG, "config.code_length differs from the bound code table");
    if (B < 1) return fail(c, GAT_ERR_ARG, "num_blocks must be positive");
    for (int p = 0; p < P; ++p)
        if (prns[p] < 0 || prns[p] >= c->P) return fail(c, GAT_ERR_RANGE, "prn outside the code table");
    const Refusal r = check_desc(sig, B, 0, signal_refusals({GAT_ERR_ARG, "chan_stride must be 0 (one signal for every PRN)"}));
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    const int layout = sig->layout;
    const int D = cfg.num_doppler_bins, J = cfg.num_code_bins, s = cfg.code_step_samples;
    const long long N = sig->num_samples;
    const int jtiles = (J + kAcqCodeTile - 1) / kAcqCodeTile, dtiles = (D + kAcqDopTile - 1) / kAcqDopTile;
    // every sample index the replica windows reach, tiles' unused code bins included
    const double reach = (double)N + kAcqChunk + (double)std::llabs((long long)cfg.first_shift) + (double)s * jtiles * kAcqCodeTile;
    if (!(reach < 1073741824.0)) return fail(c, GAT_ERR_RANGE, "N + |first_shift| + s * J must stay below 2^30 samples");
    const double ratio = cfg.code_freq_hz / fs;
    if (!code_span_ok(ratio, (double)cfg.code_length, reach, c->Lc)) return fail(c, GAT_ERR_RANGE, "code phase span too large");

    // groups of (antenna, block) units: enough workgroups for two per compute unit, within the scratch bound
    const long long cells = (long long)P * D * J;
    const long long units = (long long)sig->num_ants * B;
    const long long wgs = (long long)P * jtiles * dtiles;
    long long G = std::min<long long>(units, std::max<long long>(1, (2ll * c->num_cus + wgs - 1) / wgs));
    G = std::min<long long>(G, std::max<long long>(1, (long long)(kMaxGroupScratch / ((size_t)cells * sizeof(float)))));
    G = std::min<long long>(G, 65535 / P);
    if (G < 1) return fail(c, GAT_ERR_RANGE, "too many PRNs for one call");

    // scratch: [prns | results | power (no caller buffer) | groups' slices (G > 1)]
    const size_t off_res = 256;
    const size_t off_pow = (off_res + (size_t)P * sizeof(gat_acq_result) + 255) & ~(size_t)255;
    const size_t pow_bytes = power_dev ? 0 : (((size_t)cells * sizeof(float) + 255) & ~(size_t)255);
    const size_t off_part = off_pow + pow_bytes;
    const size_t bytes = off_part + (G > 1 ? (size_t)G * cells * sizeof(float) : 0) + (size_t)P * sizeof(int32_t);
    const size_t off_prn = bytes - (size_t)P * sizeof(int32_t);
    GAT_ENTER(c, "gat_acquire");
    {
        const int32_t rc = ensure_partial(c, bytes);
        if (rc != GAT_OK) return rc;
    }
    unsigned char *scr = reinterpret_cast<unsigned char *>(c->d_partial);
    int *d_prns = reinterpret_cast<int *>(scr + off_prn);
    gat_acq_result *d_res = reinterpret_cast<gat_acq_result *>(scr + off_res);
    float *power = power_dev ? power_dev : reinterpret_cast<float *>(scr + off_pow);
    GAT_HIP(c, hipMemcpyAsync(d_prns, prns, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));

    AcqArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.M = sig->num_ants;
    a.B = B;
    a.N = N;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.codes = c->d_codes;
    a.code_row_stride = c->code_row_stride;
    a.Lc = c->Lc;
    a.prns = d_prns;
    a.P = P;
    a.D = D;
    a.J = J;
    a.s = s;
    a.G = (int)G;
    a.ratio = ratio;
    a.fs = fs;
    a.if_hz = cfg.if_hz;
    a.f_first = cfg.doppler_first_hz;
    a.f_step = cfg.doppler_step_hz;
    a.first_shift = cfg.first_shift;
    a.out = G > 1 ? reinterpret_cast<float *>(scr + off_part) : power;
    GAT_HIP(c, acq_grid_allow_lds(s));
    GAT_HIP(c, launch_acq_grid(a, layout, c->stream));
    if (G > 1) GAT_HIP(c, launch_acq_sum_groups(a.out, power, cells, (int)G, c->stream));
    GAT_HIP(c, launch_acq_stats(power, P, D, J, cfg, fs, N, d_prns, d_res, c->stream));
    GAT_HIP(c, hipMemcpyAsync(res, d_res, (size_t)P * sizeof(gat_acq_result), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(c, hipStreamSynchronize(c->stream));
    return GAT_OK;
}
