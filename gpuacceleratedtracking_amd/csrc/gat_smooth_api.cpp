// gat_smooth_api.cpp -- host side of the carrier smoothing (include/gat.h gat_smooth_observables, gat_smooth_observables_host,
// gat_smooth_observables_plan): the four launches behind the pure plan of gat_smooth_plan.h and the host twin (the loops are
// sm_host_run, gat_smooth_plan.h).
#include "gat_ctx.h"
#include "gat_smooth_kernels.h"

using namespace gat;

GAT_API int32_t gat_smooth_observables_plan(int32_t E, int32_t K, const gat_smooth_config *cfg, gat_smooth_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_smooth_plan)) return GAT_ERR_ARG;
    // stand-ins for the pointers the plan only compares with null
    const SmIn in{reinterpret_cast<const int32_t *>(out), reinterpret_cast<const double *>(out), reinterpret_cast<const int32_t *>(out),
                  reinterpret_cast<const double *>(out), reinterpret_cast<const int64_t *>(out), reinterpret_cast<const double *>(out),
                  reinterpret_cast<const double *>(out), nullptr};
    SmOut o{};
    o.tx_frac_out = reinterpret_cast<double *>(out);
    SmPlan plan{};
    const Refusal r = sm_plan(SmCall{in, E, K, cfg, o}, &plan);
    if (r.code != GAT_OK) return r.code;
    sm_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_smooth_observables(gat_ctx *c, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms, const double *rx_frac,
                                       const int64_t *carrier_cycles, const double *carrier_frac, const double *doppler_hz, const uint8_t *valid,
                                       int32_t E, int32_t K, const gat_smooth_config *cfg, double *tx_frac_out, int32_t *count, double *cmc_s,
                                       uint8_t *status, gat_smooth_channel *channels)
{
    if (!c) return GAT_ERR_ARG;
    const SmIn in{tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, valid};
    const SmOut out{tx_frac_out, count, cmc_s, status, channels};
    SmPlan p{};
    const Refusal r = sm_plan(SmCall{in, E, K, cfg, out}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_smooth_observables");
    const int32_t rc = ensure_partial(c, p.bytes);
    if (rc != GAT_OK) return rc;
    char *scratch = reinterpret_cast<char *>(c->d_partial);
    SmArgs a{};
    a.in = in, a.out = out, a.rule = p.rule;
    a.E = p.E, a.K = p.K, a.chunks = p.chunks, a.lanes = p.lanes, a.rows = p.rows, a.run = p.run, a.cells = p.cells;
    a.totals = reinterpret_cast<SmSeg *>(scratch + p.off_totals);
    a.runs = reinterpret_cast<SmSeg *>(scratch + p.off_runs);
    a.C = reinterpret_cast<uint64_t *>(scratch + p.off_C);
    a.SS = reinterpret_cast<uint64_t *>(scratch + p.off_SS);
    a.arc = reinterpret_cast<int32_t *>(scratch + p.off_arc);
    GAT_HIP(c, launch_smooth(a, p, c->stream));
    set_last_launch(c, p.chunks, kSmThreads, p.chunks, 1, kSmLdsBytes);
    return GAT_OK;
}

GAT_API int32_t gat_smooth_observables_host(const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms, const double *rx_frac,
                                            const int64_t *carrier_cycles, const double *carrier_frac, const double *doppler_hz,
                                            const uint8_t *valid, int32_t E, int32_t K, const gat_smooth_config *cfg, double *tx_frac_out,
                                            int32_t *count, double *cmc_s, uint8_t *status, gat_smooth_channel *channels)
{
    const SmIn in{tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, valid};
    const SmOut out{tx_frac_out, count, cmc_s, status, channels};
    SmPlan p{};
    const Refusal r = sm_plan(SmCall{in, E, K, cfg, out}, &p);
    if (r.code != GAT_OK) return r.code;
    sm_host_run(p, in, out);
    return GAT_OK;
}
