// gat_nav_api.cpp -- host side of the navigation data layer (include/gat.h gat_nav_decode, gat_nav_decode_host, gat_nav_decode_plan):
// the launch sequence behind the pure plan of gat_nav_plan.h -- {slice | quantise, trellis}; {scores, choice}; frames, each only
// where an output needs it --, and the host twin (the loops are nav_host_run, gat_nav_plan.h).
#include "gat_ctx.h"
#include "gat_nav_kernels.h"

using namespace gat;

GAT_API int32_t gat_nav_decode_plan(int32_t K, const gat_nav_config *cfg, gat_nav_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_nav_plan)) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plan only compares with null
    NavPlan plan{};
    const Refusal r = nav_plan(NavCall{given, nullptr, K, cfg, given, given, given, given}, &plan);
    if (r.code != GAT_OK) return r.code;
    nav_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_nav_decode(gat_ctx *c, const double *sym_re, const gat_monitor_channel *mon, int32_t K, const gat_nav_config *cfg,
                               gat_nav_channel *channels, gat_nav_frame *frames, uint8_t *decoded, int32_t *path_metric)
{
    if (!c) return GAT_ERR_ARG;
    NavPlan p{};
    const Refusal r = nav_plan(NavCall{sym_re, mon, K, cfg, channels, frames, decoded, path_metric}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_nav_decode");
    if (p.bytes > 0) {
        const int32_t rc = ensure_partial(c, p.bytes);
        if (rc != GAT_OK) return rc;
    }
    char *scratch = reinterpret_cast<char *>(c->d_partial);
    NavArgs a{};
    a.sym_re = sym_re, a.mon = mon;
    a.q = reinterpret_cast<int8_t *>(scratch + p.off_q);
    a.surv = reinterpret_cast<unsigned long long *>(scratch + p.off_surv);
    a.decoded = p.own_decoded ? reinterpret_cast<uint8_t *>(scratch + p.off_decoded) : decoded;
    a.scores = reinterpret_cast<int32_t *>(scratch + p.off_scores);
    a.chan = p.own_chan ? reinterpret_cast<gat_nav_channel *>(scratch + p.off_chan) : channels;
    a.frames = frames, a.path_metric = path_metric;
    a.format = p.format, a.K = p.K, a.cap = p.cap, a.P = p.P, a.bit_cap = p.bit_cap, a.max_frames = p.max_frames, a.min_frames = p.min_frames, a.C = p.C;
    if (p.g_slice) GAT_HIP(c, launch_nav_slice(a, p.g_slice, c->stream));
    if (p.g_quant) GAT_HIP(c, launch_nav_quantise(a, p.g_quant, c->stream));
    if (p.g_trellis) GAT_HIP(c, launch_nav_trellis(a, p.g_trellis, c->stream));
    if (p.g_score) GAT_HIP(c, launch_nav_score(a, p.g_score, c->stream));
    if (p.g_pick) GAT_HIP(c, launch_nav_pick(a, p.g_pick, c->stream));
    if (p.g_frame) GAT_HIP(c, launch_nav_frames(a, p.g_frame, c->stream));
    set_last_launch(c, p.g_trellis ? p.g_trellis : p.g_slice, p.g_trellis ? kNavWave : kNavThreads, 1, 1, 0);
    return GAT_OK;
}

GAT_API int32_t gat_nav_decode_host(const double *sym_re, const gat_monitor_channel *mon, int32_t K, const gat_nav_config *cfg,
                                    gat_nav_channel *channels, gat_nav_frame *frames, uint8_t *decoded, int32_t *path_metric)
{
    NavPlan p{};
    const Refusal r = nav_plan(NavCall{sym_re, mon, K, cfg, channels, frames, decoded, path_metric}, &p);
    if (r.code != GAT_OK) return r.code;
    nav_host_run(p, sym_re, mon, channels, frames, decoded, path_metric);
    return GAT_OK;
}
