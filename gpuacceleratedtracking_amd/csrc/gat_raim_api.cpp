// gat_raim_api.cpp -- host side of the fix integrity (include/gat.h gat_position_fix_raim, gat_position_fix_raim_host,
// gat_position_fix_raim_plan): the one launch behind the pure plan of gat_raim_plan.h and the host twin (the loops are raim_host_run,
// gat_raim_plan.h).
#include "gat_ctx.h"
#include "gat_raim_kernels.h"

using namespace gat;

GAT_API int32_t gat_position_fix_raim_plan(int32_t E, int32_t K, const gat_fix_config *cfg, const gat_raim_config *raim, gat_fix_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_fix_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    RaimPlan plan{};
    const Refusal r = raim_plan(RaimCall{FixCall{given, given, given, given, given, E, K, cfg, given}, raim, given}, &plan);
    if (r.code != GAT_OK) return r.code;
    raim_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_position_fix_raim(gat_ctx *c, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                                      const double *rx_frac, const double *weights, int32_t E, int32_t K, const gat_fix_config *cfg,
                                      const gat_raim_config *raim, gat_fix *fixes, gat_fix_integrity *integrity, double *sat, double *resid,
                                      double *sin_el, uint8_t *used, double *trial)
{
    if (!c) return GAT_ERR_ARG;
    RaimPlan p{};
    const Refusal r = raim_plan(RaimCall{FixCall{eph, tx_ms, tx_frac, rx_ms, rx_frac, E, K, cfg, fixes}, raim, integrity}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_position_fix_raim");
    RaimArgs a{};
    a.fix = fix_args(p.fix, eph, tx_ms, tx_frac, rx_ms, rx_frac, weights, fixes, sat, resid, sin_el, used);
    a.integrity = integrity, a.trial = trial;
    a.max_exclude = p.max_exclude, a.trial_iter = p.trial_iter;
    for (int d = 0; d < kRaimThresholds; ++d) a.threshold[d] = p.threshold[d];
    GAT_HIP(c, launch_raim(a, p.fix.groups, c->stream));
    set_last_launch(c, p.fix.groups, kFixThreads, 1, 1, kRaimLdsBytes);
    return GAT_OK;
}

GAT_API int32_t gat_position_fix_raim_host(const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                                           const double *rx_frac, const double *weights, int32_t E, int32_t K, const gat_fix_config *cfg,
                                           const gat_raim_config *raim, gat_fix *fixes, gat_fix_integrity *integrity, double *sat, double *resid,
                                           double *sin_el, uint8_t *used, double *trial)
{
    RaimPlan p{};
    const Refusal r = raim_plan(RaimCall{FixCall{eph, tx_ms, tx_frac, rx_ms, rx_frac, E, K, cfg, fixes}, raim, integrity}, &p);
    if (r.code != GAT_OK) return r.code;
    raim_host_run(p, eph, tx_ms, tx_frac, rx_ms, rx_frac, weights, fixes, integrity, sat, resid, sin_el, used, trial);
    return GAT_OK;
}
