// gat_snap_api.cpp -- host side of the snapshot fix (include/gat.h gat_snapshot_fix, gat_snapshot_fix_host, gat_snapshot_fix_plan):
// the one launch behind the pure plan of gat_snap_plan.h and the host twin (the loops are snap_host_run, gat_snap_plan.h).
#include "gat_ctx.h"
#include "gat_snap_kernels.h"

using namespace gat;

GAT_API int32_t gat_snapshot_fix_plan(int32_t E, int32_t K, const gat_snap_config *cfg, gat_fix_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_fix_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    SnapPlan plan{};
    const Refusal r = snap_plan(SnapCall{given, given, given, given, E, K, cfg, given}, &plan);
    if (r.code != GAT_OK) return r.code;
    snap_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_snapshot_fix(gat_ctx *c, const gat_ephemeris *eph, const double *code_frac, const int32_t *rx_ms, const double *rx_frac,
                                 const double *prior_xyz, const double *weights, int32_t E, int32_t K, const gat_snap_config *cfg,
                                 gat_snap_fix *fixes, int32_t *tx_ms, int32_t *rx_ms_out, int32_t *n_ms, double *resid, double *sin_el,
                                 uint8_t *used)
{
    if (!c) return GAT_ERR_ARG;
    SnapPlan p{};
    const Refusal r = snap_plan(SnapCall{eph, code_frac, rx_ms, rx_frac, E, K, cfg, fixes}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_snapshot_fix");
    SnapArgs a{};
    a.eph = eph, a.code_frac = code_frac, a.rx_ms = rx_ms, a.rx_frac = rx_frac, a.prior = prior_xyz, a.w = weights;
    a.fixes = fixes, a.tx_ms = tx_ms, a.rx_ms_out = rx_ms_out, a.n_ms = n_ms, a.resid = resid, a.sin_el = sin_el, a.used = used;
    a.E = p.E, a.K = p.K, a.max_iter = p.max_iter, a.tol_m = p.tol_m, a.mask_sin = p.mask_sin, a.margin = p.margin;
    for (int i = 0; i < 3; ++i) a.init_xyz[i] = p.init_xyz[i];
    GAT_HIP(c, launch_snap(a, p.groups, c->stream));
    set_last_launch(c, p.groups, kFixThreads, 1, 1, kSnapLdsBytes);
    return GAT_OK;
}

GAT_API int32_t gat_snapshot_fix_host(const gat_ephemeris *eph, const double *code_frac, const int32_t *rx_ms, const double *rx_frac,
                                      const double *prior_xyz, const double *weights, int32_t E, int32_t K, const gat_snap_config *cfg,
                                      gat_snap_fix *fixes, int32_t *tx_ms, int32_t *rx_ms_out, int32_t *n_ms, double *resid, double *sin_el,
                                      uint8_t *used)
{
    SnapPlan p{};
    const Refusal r = snap_plan(SnapCall{eph, code_frac, rx_ms, rx_frac, E, K, cfg, fixes}, &p);
    if (r.code != GAT_OK) return r.code;
    snap_host_run(p, eph, code_frac, rx_ms, rx_frac, prior_xyz, weights, fixes, tx_ms, rx_ms_out, n_ms, resid, sin_el, used);
    return GAT_OK;
}
