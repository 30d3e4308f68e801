// gat_atm_api.cpp -- host side of the range corrections (include/gat.h gat_range_corrections, gat_range_corrections_host,
// gat_range_corrections_plan, gat_atm_atan2_host, gat_lnav_page18_host, gat_lnav_page18_words_host): the one launch behind the pure
// plan of gat_atm_plan.h, the host twin (the loops are atm_host_run, gat_atm_plan.h) and the decoder and encoder of subframe 4,
// page 18 (gat_atm_page18.h).
#include "gat_ctx.h"
#include "gat_atm_kernels.h"
#include "gat_atm_page18.h"

using namespace gat;

GAT_API int32_t gat_range_corrections_plan(int32_t E, int32_t K, const gat_atm_config *cfg, gat_fix_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_fix_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    AtmPlan plan{};
    const Refusal r = atm_plan(AtmCall{given, given, given, given, given, given, E, K, cfg, given}, &plan);
    if (r.code != GAT_OK) return r.code;
    atm_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_range_corrections(gat_ctx *c, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                                      const double *rx_frac, const gat_fix *fixes, const double *zenith, int32_t E, int32_t K,
                                      const gat_atm_config *cfg, double *tx_frac_out, double *delay, double *geom, uint8_t *channel_status,
                                      int32_t *epoch_status)
{
    if (!c) return GAT_ERR_ARG;
    AtmPlan p{};
    const Refusal r = atm_plan(AtmCall{eph, tx_ms, tx_frac, rx_ms, rx_frac, fixes, E, K, cfg, tx_frac_out}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_range_corrections");
    AtmArgs a{};
    a.eph = eph, a.tx_ms = tx_ms, a.tx_frac = tx_frac, a.rx_ms = rx_ms, a.rx_frac = rx_frac, a.fixes = fixes, a.zenith = zenith;
    a.tx_frac_out = tx_frac_out, a.delay = delay, a.geom = geom, a.ch_status = channel_status, a.ep_status = epoch_status;
    a.K = p.K, a.cells = p.cells, a.prm = p.prm;
    GAT_HIP(c, launch_atm(a, p.groups, c->stream));
    set_last_launch(c, p.groups, kAtmThreads, 1, 1, 0);
    return GAT_OK;
}

GAT_API int32_t gat_range_corrections_host(const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                                           const double *rx_frac, const gat_fix *fixes, const double *zenith, int32_t E, int32_t K,
                                           const gat_atm_config *cfg, double *tx_frac_out, double *delay, double *geom, uint8_t *channel_status,
                                           int32_t *epoch_status)
{
    AtmPlan p{};
    const Refusal r = atm_plan(AtmCall{eph, tx_ms, tx_frac, rx_ms, rx_frac, fixes, E, K, cfg, tx_frac_out}, &p);
    if (r.code != GAT_OK) return r.code;
    atm_host_run(p, eph, tx_ms, tx_frac, rx_ms, rx_frac, fixes, zenith, tx_frac_out, delay, geom, channel_status, epoch_status);
    return GAT_OK;
}

GAT_API int32_t gat_atm_atan2_host(const double *y, const double *x, int64_t count, double *angle)
{
    if (!y || !x || !angle || count < 0) return GAT_ERR_ARG;
    for (int64_t i = 0; i < count; ++i) angle[i] = atm_atan2(y[i], x[i]);
    return GAT_OK;
}

GAT_API int32_t gat_lnav_page18_host(const gat_nav_frame *frames, int32_t num_frames, gat_lnav_page18 *page)
{
    if (!page || num_frames < 0 || (!frames && num_frames > 0)) return GAT_ERR_ARG;
    page18_decode(frames, num_frames, page);
    return GAT_OK;
}

GAT_API int32_t gat_lnav_page18_words_host(const gat_lnav_page18 *page, uint8_t *payload_bits)
{
    if (!page || !payload_bits) return GAT_ERR_ARG;
    page18_encode(page, payload_bits);
    return GAT_OK;
}
