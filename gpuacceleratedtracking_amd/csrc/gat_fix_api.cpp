// gat_fix_api.cpp -- host side of the position fix (include/gat.h gat_position_fix, gat_position_fix_host, gat_position_fix_plan,
// gat_lnav_ephemeris_host, gat_lnav_ephemeris_words_host): the one launch behind the pure plan of gat_fix_plan.h, the host twin (the
// loops are fix_host_run, gat_fix_plan.h) and the ephemeris decoder and encoder (gat_fix_eph.h).
#include "gat_ctx.h"
#include "gat_fix_eph.h"
#include "gat_fix_kernels.h"

using namespace gat;

GAT_API int32_t gat_position_fix_plan(int32_t E, int32_t K, const gat_fix_config *cfg, gat_fix_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_fix_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    FixPlan plan{};
    const Refusal r = fix_plan(FixCall{given, given, given, given, given, E, K, cfg, given}, &plan);
    if (r.code != GAT_OK) return r.code;
    fix_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_position_fix(gat_ctx *c, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                                 const double *rx_frac, const double *weights, int32_t E, int32_t K, const gat_fix_config *cfg, gat_fix *fixes,
                                 double *sat, double *resid, double *sin_el, uint8_t *used)
{
    if (!c) return GAT_ERR_ARG;
    FixPlan p{};
    const Refusal r = fix_plan(FixCall{eph, tx_ms, tx_frac, rx_ms, rx_frac, E, K, cfg, fixes}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_position_fix");
    const FixArgs a = fix_args(p, eph, tx_ms, tx_frac, rx_ms, rx_frac, weights, fixes, sat, resid, sin_el, used);
    GAT_HIP(c, launch_fix(a, p.groups, c->stream));
    set_last_launch(c, p.groups, kFixThreads, 1, 1, kFixLdsBytes);
    return GAT_OK;
}

GAT_API int32_t gat_position_fix_host(const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                                      const double *rx_frac, const double *weights, int32_t E, int32_t K, const gat_fix_config *cfg,
                                      gat_fix *fixes, double *sat, double *resid, double *sin_el, uint8_t *used)
{
    FixPlan p{};
    const Refusal r = fix_plan(FixCall{eph, tx_ms, tx_frac, rx_ms, rx_frac, E, K, cfg, fixes}, &p);
    if (r.code != GAT_OK) return r.code;
    fix_host_run(p, eph, tx_ms, tx_frac, rx_ms, rx_frac, weights, fixes, sat, resid, sin_el, used);
    return GAT_OK;
}

GAT_API int32_t gat_lnav_ephemeris_host(const gat_nav_frame *frames, int32_t num_frames, gat_ephemeris *eph)
{
    if (!eph || num_frames < 0 || (!frames && num_frames > 0)) return GAT_ERR_ARG;
    eph_decode(frames, num_frames, eph);
    return GAT_OK;
}

GAT_API int32_t gat_lnav_ephemeris_words_host(const gat_ephemeris *eph, uint8_t *payload_bits)
{
    if (!eph || !payload_bits) return GAT_ERR_ARG;
    eph_encode(eph, payload_bits);
    return GAT_OK;
}
