// gat_fir_api.cpp -- host side of the sample filter (include/gat.h gat_filter_samples): the launch behind the pure plan of
// gat_fir_plan.h, and the host twin (gat_filter_samples_host), which runs the loop of gat_fir.h.  The kernels are gat_fir.hip.
#include "gat_ctx.h"
#include "gat_fir_kernels.h"

using namespace gat;

GAT_API int32_t gat_filter_samples(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const float *taps_re, const float *taps_im,
                                   const gat_fir_config *cfg, const gat_signal_desc *out)
{
    if (!c) return GAT_ERR_ARG;
    FirPlan plan{};
    const Refusal r = fir_plan(sig, B, taps_re, taps_im, cfg, out, (long long)c->num_cus * 8, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_filter_samples");
    FirArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.out_re = static_cast<float *>(const_cast<void *>(out->re));
    a.out_im = static_cast<float *>(const_cast<void *>(out->im));
    a.taps_re = taps_re;
    a.taps_im = taps_im;
    a.M = sig->num_ants;
    a.T = cfg->num_taps;
    a.D = cfg->decimation;
    a.tile = plan.tile;
    a.row = plan.row;
    a.N = sig->num_samples;
    a.Q = plan.Q;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.out_ant_stride = out->ant_stride;
    a.out_block_stride = out->block_stride;
    a.chunk = plan.chunk;
    a.chunks = plan.chunks;
    a.units = plan.units;
    a.nco = fir_nco(cfg->nco_step, cfg->nco_phase);
    GAT_HIP(c, plan.tiled ? launch_fir_tiled(a, sig->layout, out->layout, (int)plan.grid, c->stream)
                          : launch_fir_general(a, sig->layout, out->layout, (int)plan.grid, c->stream));
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)plan.grid;
    c->last.threads = kFirThreads;
    c->last.splits = (int32_t)plan.chunks;
    c->last.ant_tile = 1; // a work unit is one antenna's
    c->last.vec = plan.tiled ? layout_vec_samples(sig->layout) : 1;
    // the tiled kernel's samples in polyphase order; the general kernel's taps
    c->last.lds_bytes = (int32_t)sizeof(float2) * (plan.tiled ? kFirLdsSamples : GAT_MAX_FIR_TAPS);
    return GAT_OK;
}

GAT_API int32_t gat_filter_samples_host(const gat_signal_desc *sig, int32_t B, const float *taps_re, const float *taps_im, const gat_fir_config *cfg,
                                        const gat_signal_desc *out)
{
    FirPlan plan{};
    const Refusal r = fir_plan(sig, B, taps_re, taps_im, cfg, out, 1, &plan);
    if (r.code != GAT_OK) return r.code;
    fir_host_run(sig, B, taps_re, taps_im, cfg->num_taps, cfg->decimation, cfg->nco_step, cfg->nco_phase, out);
    return GAT_OK;
}
