// gat_obs_api.cpp -- host side of the observables (include/gat.h gat_tracking_run_history, gat_observables, gat_observables_host,
// gat_observables_plan): the loop's run that keeps every block's parameters, the four launches behind the pure plan of
// gat_obs_plan.h and the host twin (the loops are obs_host_run, gat_obs_plan.h).
#include "gat_ctx.h"
#include "gat_obs_kernels.h"

using namespace gat;

// The sequence of gat_tracking_run (tracking_run_enqueue, gat_api.cpp) with the ping-pong pair replaced by the rows of one array:
// block b is correlated with history + b K and its update writes history + (b + 1) K.  Its own checks and trace range; the same
// launches and bits as the runs that keep two buffers.
GAT_API int32_t gat_tracking_run_history(gat_ctx *c, const gat_signal_desc *sig, int32_t num_blocks, int32_t K, int32_t L, const int32_t *shifts,
                                         double fs, const gat_loop_config *cfg, gat_loop_state *state, gat_channel_params *history,
                                         float *acc_re, float *acc_im, int64_t acc_block_stride, uint32_t flags, const double *w_re,
                                         const double *w_im)
{
    if (!c || !sig || !shifts || !cfg || !state || !history || !acc_re || !acc_im) return fail(c, GAT_ERR_ARG, "null argument");
    if ((w_re == nullptr) != (w_im == nullptr)) return fail(c, GAT_ERR_ARG, "one weight pointer without the other");
    if (num_blocks < 1 || acc_block_stride < 0 || K < 1) return fail(c, GAT_ERR_ARG, "bad block count / stride");
    if (cfg->num_taps != L || L < 1 || L > GAT_MAX_TAPS) return fail(c, GAT_ERR_ARG, "loop configuration and tap list disagree");
    if (flags & GAT_FLAG_GRAPH) return fail(c, GAT_ERR_ARG, "the history run is not replayed as a graph");
    if (flags & ~GAT_FLAG_ATOMIC) return fail(c, GAT_ERR_ARG, "unknown flag bits");
    GAT_ENTER(c, "gat_tracking_run_history");
    return tracking_run_enqueue(c, sig, num_blocks, K, L, shifts, fs, cfg, state, LoopRecords{history, nullptr}, acc_re, acc_im, acc_block_stride,
                                flags, w_re, w_im);
}

GAT_API int32_t gat_observables_plan(int32_t B, int32_t K, int32_t E, const gat_obs_config *cfg, gat_obs_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_obs_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    ObsOut o{};
    o.channels = reinterpret_cast<gat_obs_channel *>(out);
    ObsPlan plan{};
    const Refusal r = obs_plan(ObsCall{given, given, given, given, B, K, E, cfg, o}, &plan);
    if (r.code != GAT_OK) return r.code;
    obs_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_observables(gat_ctx *c, const gat_channel_params *history, const gat_monitor_channel *mon, const gat_nav_channel *nav,
                                const gat_nav_frame *frames, int32_t B, int32_t K, int32_t E, const gat_obs_config *cfg, int32_t *tx_ms,
                                double *tx_frac, int32_t *rx_ms, double *rx_frac, int64_t *carrier_cycles, double *carrier_frac,
                                double *doppler_hz, double *code_rate_hz, gat_obs_channel *channels)
{
    if (!c) return GAT_ERR_ARG;
    const ObsOut out{tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, code_rate_hz, channels};
    ObsPlan p{};
    const Refusal r = obs_plan(ObsCall{history, mon, nav, frames, B, K, E, cfg, out}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_observables");
    const int32_t rc = ensure_partial(c, p.bytes);
    if (rc != GAT_OK) return rc;
    char *scratch = reinterpret_cast<char *>(c->d_partial);
    ObsArgs a{};
    a.hist = history, a.mon = mon, a.nav = nav, a.frames = frames, a.out = out, a.rule = p.rule;
    a.chunks = p.chunks, a.group = p.group, a.groups = p.groups, a.lanes = p.lanes, a.rows = p.rows, a.run = p.run;
    a.totals = reinterpret_cast<ObsSum *>(scratch + p.off_totals);
    a.bad = reinterpret_cast<int32_t *>(scratch + p.off_bad);
    a.runs = reinterpret_cast<ObsSum *>(scratch + p.off_runs);
    a.chan = reinterpret_cast<ObsChan *>(scratch + p.off_chan);
    a.anchor = reinterpret_cast<ObsAnchor *>(scratch + p.off_anchor);
    GAT_HIP(c, launch_obs(a, p, c->stream));
    set_last_launch(c, p.chunk_groups, kObsThreads, p.chunks, 1, kObsLdsBytes);
    return GAT_OK;
}

GAT_API int32_t gat_observables_host(const gat_channel_params *history, const gat_monitor_channel *mon, const gat_nav_channel *nav,
                                     const gat_nav_frame *frames, int32_t B, int32_t K, int32_t E, const gat_obs_config *cfg, int32_t *tx_ms,
                                     double *tx_frac, int32_t *rx_ms, double *rx_frac, int64_t *carrier_cycles, double *carrier_frac,
                                     double *doppler_hz, double *code_rate_hz, gat_obs_channel *channels)
{
    const ObsOut out{tx_ms, tx_frac, rx_ms, rx_frac, carrier_cycles, carrier_frac, doppler_hz, code_rate_hz, channels};
    ObsPlan p{};
    const Refusal r = obs_plan(ObsCall{history, mon, nav, frames, B, K, E, cfg, out}, &p);
    if (r.code != GAT_OK) return r.code;
    obs_host_run(p, history, mon, nav, frames, out);
    return GAT_OK;
}
