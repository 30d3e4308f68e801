// gat_acq_api.cpp -- host side of the direct acquisition search (include/gat.h gat_acquire, gat_acq_stats_host): the grid launch
// behind the pure plan of gat_acq_plan.h, inside the frame both searches share (gat_acq_frame.h), and the statistics on the host
// (csrc/gat_acq.h).
#include <algorithm>
#include <limits>
#include <vector>

#include "gat_acq.h"
#include "gat_acq_frame.h"

using namespace gat;

namespace {

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
    const Refusal r = acq_check_config(cfg, P, D, J, fs);
    if (r.code != GAT_OK) return r.code;
    if (cfg->code_length < 1) return GAT_ERR_ARG;
    if (N < 1) return GAT_ERR_ARG;
    stats_host(power, P, D, J, *cfg, fs, (long long)N, res);
    return GAT_OK;
}

GAT_API int32_t gat_acquire(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const int32_t *prns, int32_t P, double fs,
                            const gat_acq_config *cfg_in, float *power_dev, gat_acq_result *res)
{
    gat_acq_config cfg;
    const int32_t rc = acq_check_entry(c, sig, B, prns, P, fs, cfg_in, res, &cfg);
    if (rc != GAT_OK) return rc;
    AcqPlan pl{};
    const Refusal r = acq_plan(sig, B, P, fs, &cfg, c->num_cus, power_dev == nullptr, &pl);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    return acq_run<AcqArgs>(c, "gat_acquire", sig, B, prns, P, fs, cfg, pl, pl.G, power_dev, res, [&](AcqArgs &a, unsigned char *) -> int32_t {
        a.G = pl.G;
        GAT_HIP(c, acq_grid_allow_lds(a.s));
        GAT_HIP(c, launch_acq_grid(a, sig->layout, c->stream));
        return GAT_OK;
    });
}

