// gat_mon_api.cpp -- host side of the tracking monitor (include/gat.h gat_track_monitor, gat_track_monitor_host,
// gat_track_monitor_plan): the launch sequence behind the pure plan of gat_mon_plan.h -- {prompts; windows; terms, energies, choice;
// symbols}, each only where an output needs it --, and the host twin (the loops are mon_host_run, gat_mon_plan.h).
#include <cstring>

#include "gat_ctx.h"
#include "gat_mon_kernels.h"

using namespace gat;

namespace {

MonCall mon_call(const float *acc_re, const float *acc_im, int64_t stride, int32_t B, int32_t K, int32_t M, const gat_monitor_config *cfg,
                 const double *w_re, const double *w_im, const double *prompt_re, const double *prompt_im, const gat_monitor_window *windows,
                 const double *energy, const gat_monitor_channel *channels, const double *sym_re, const double *sym_im, const double *sym_wbp)
{
    return MonCall{acc_re, acc_im, stride, B, K, M, cfg, w_re, w_im, prompt_re, prompt_im, windows, energy, channels, sym_re, sym_im, sym_wbp};
}

} // namespace

GAT_API int32_t gat_track_monitor_plan(int64_t stride, int32_t B, int32_t K, int32_t M, const gat_monitor_config *cfg, int32_t own_prompts,
                                       int32_t want_symbols, gat_monitor_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_monitor_plan)) return GAT_ERR_ARG;
    // stand-ins for the pointers the plan only compares with null
    const void *const given = out;
    MonCall a{given, given, stride, B, K, M, cfg, nullptr, nullptr, own_prompts ? nullptr : given, own_prompts ? nullptr : given, given,
              want_symbols ? given : nullptr, want_symbols ? given : nullptr, want_symbols ? given : nullptr, want_symbols ? given : nullptr,
              want_symbols ? given : nullptr};
    MonPlan plan{};
    const Refusal r = mon_plan(a, &plan);
    if (r.code != GAT_OK) return r.code;
    mon_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_track_monitor(gat_ctx *c, const float *acc_re, const float *acc_im, int64_t stride, int32_t B, int32_t K, int32_t M,
                                  const gat_monitor_config *cfg, const double *w_re, const double *w_im, double *prompt_re, double *prompt_im,
                                  gat_monitor_window *windows, double *energy, gat_monitor_channel *channels, double *sym_re, double *sym_im,
                                  double *sym_wbp)
{
    if (!c) return GAT_ERR_ARG;
    MonPlan p{};
    const Refusal r = mon_plan(mon_call(acc_re, acc_im, stride, B, K, M, cfg, w_re, w_im, prompt_re, prompt_im, windows, energy, channels, sym_re, sym_im, sym_wbp), &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_track_monitor");
    if (p.bytes > 0) {
        const int32_t rc = ensure_partial(c, p.bytes);
        if (rc != GAT_OK) return rc;
    }
    char *scratch = reinterpret_cast<char *>(c->d_partial);
    MonArgs a{};
    a.acc_re = acc_re, a.acc_im = acc_im, a.acc_block_stride = B > 1 ? stride : 0;
    a.w_re = w_re, a.w_im = w_im;
    a.pr = p.own_pr ? reinterpret_cast<double *>(scratch + p.off_pr) : prompt_re;
    a.pi = p.own_pi ? reinterpret_cast<double *>(scratch + p.off_pi) : prompt_im;
    a.terms = reinterpret_cast<double *>(scratch + p.off_terms);
    a.energy = p.own_energy ? reinterpret_cast<double *>(scratch + p.off_energy) : energy;
    a.chan = p.own_chan ? reinterpret_cast<gat_monitor_channel *>(scratch + p.off_chan) : channels;
    a.windows = windows;
    a.sym_re = sym_re, a.sym_im = sym_im, a.sym_wbp = sym_wbp;
    a.B = p.B, a.K = p.K, a.M = p.M, a.L = p.L, a.prompt = p.prompt, a.W = p.W, a.Pd = p.Pd, a.forced = p.forced;
    a.first_block = p.first_block, a.NW = p.NW, a.J = p.J, a.cap = p.cap;
    std::memcpy(a.overlay, cfg->overlay, sizeof(a.overlay));
    GAT_HIP(c, launch_mon_prompts(a, p.g_prompt, c->stream));
    if (p.g_window) GAT_HIP(c, launch_mon_windows(a, p.g_window, c->stream));
    if (p.g_term) GAT_HIP(c, launch_mon_terms(a, p.g_term, c->stream));
    if (p.g_energy) GAT_HIP(c, launch_mon_energies(a, p.g_energy, c->stream));
    if (p.g_pick) GAT_HIP(c, launch_mon_pick(a, p.g_pick, c->stream));
    if (p.g_symbol) GAT_HIP(c, launch_mon_symbols(a, p.g_symbol, c->stream));
    set_last_launch(c, p.g_prompt, kMonThreads, 1, p.M, p.g_window ? (int32_t)(2 * kMonThreads * sizeof(double)) : 0);
    return GAT_OK;
}

GAT_API int32_t gat_track_monitor_host(const float *acc_re, const float *acc_im, int64_t stride, int32_t B, int32_t K, int32_t M,
                                       const gat_monitor_config *cfg, const double *w_re, const double *w_im, double *prompt_re, double *prompt_im,
                                       gat_monitor_window *windows, double *energy, gat_monitor_channel *channels, double *sym_re, double *sym_im,
                                       double *sym_wbp)
{
    MonPlan p{};
    const Refusal r = mon_plan(mon_call(acc_re, acc_im, stride, B, K, M, cfg, w_re, w_im, prompt_re, prompt_im, windows, energy, channels, sym_re, sym_im, sym_wbp), &p);
    if (r.code != GAT_OK) return r.code;
    mon_host_run(p, acc_re, acc_im, stride, cfg, w_re, w_im, prompt_re, prompt_im, windows, energy, channels, sym_re, sym_im, sym_wbp);
    return GAT_OK;
}
