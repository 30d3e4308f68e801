// gat_vel_api.cpp -- host side of the velocity fix (include/gat.h gat_velocity_fix, gat_velocity_fix_host, gat_velocity_fix_plan):
// the one launch behind the pure plan of gat_vel_plan.h and the host twin (the loops are vel_host_run, gat_vel_plan.h).
#include "gat_ctx.h"
#include "gat_vel_kernels.h"

using namespace gat;

GAT_API int32_t gat_velocity_fix_plan(int32_t E, int32_t K, const gat_vel_config *cfg, gat_fix_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_fix_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    VelPlan plan{};
    const Refusal r = vel_plan(VelCall{given, given, given, given, given, E, K, cfg, given}, &plan);
    if (r.code != GAT_OK) return r.code;
    vel_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_velocity_fix(gat_ctx *c, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const double *doppler,
                                 const gat_fix *fixes, const uint8_t *used, const double *weights, int32_t E, int32_t K,
                                 const gat_vel_config *cfg, gat_velocity *vel, double *sat_vel, double *resid)
{
    if (!c) return GAT_ERR_ARG;
    VelPlan p{};
    const Refusal r = vel_plan(VelCall{eph, tx_ms, tx_frac, doppler, fixes, E, K, cfg, vel}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_velocity_fix");
    VelArgs a{};
    a.eph = eph, a.tx_ms = tx_ms, a.tx_frac = tx_frac, a.doppler = doppler, a.fixes = fixes, a.used_in = used, a.w = weights;
    a.vel = vel, a.sat_vel = sat_vel, a.resid = resid;
    a.E = p.E, a.K = p.K, a.lambda = p.lambda;
    GAT_HIP(c, launch_vel(a, p.groups, c->stream));
    set_last_launch(c, p.groups, kFixThreads, 1, 1, kFixLdsBytes);
    return GAT_OK;
}

GAT_API int32_t gat_velocity_fix_host(const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const double *doppler,
                                      const gat_fix *fixes, const uint8_t *used, const double *weights, int32_t E, int32_t K,
                                      const gat_vel_config *cfg, gat_velocity *vel, double *sat_vel, double *resid)
{
    VelPlan p{};
    const Refusal r = vel_plan(VelCall{eph, tx_ms, tx_frac, doppler, fixes, E, K, cfg, vel}, &p);
    if (r.code != GAT_OK) return r.code;
    vel_host_run(p, eph, tx_ms, tx_frac, doppler, fixes, used, weights, vel, sat_vel, resid);
    return GAT_OK;
}
