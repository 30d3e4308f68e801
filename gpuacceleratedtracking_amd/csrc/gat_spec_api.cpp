// gat_spec_api.cpp -- host side of the sample spectrum (include/gat.h gat_sample_spectrum): the launch behind the pure plan of
// gat_spec_plan.h, and the host twin (gat_sample_spectrum_host), which runs the loop of gat_spec.h.  The kernels are gat_spec.hip.
#include "gat_ctx.h"
#include "gat_spec_kernels.h"

using namespace gat;

GAT_API int32_t gat_sample_spectrum(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const float *window, const gat_spectrum_config *cfg, float *power)
{
    if (!c) return GAT_ERR_ARG;
    SpecPlan plan{};
    // a workgroup holds its unit for all its segments: eight workgroups a compute unit keep every SIMD busy through the barriers
    const Refusal r = spec_plan(sig, B, window, cfg, power, (long long)c->num_cus * 8, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_sample_spectrum");
    SpecArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.window = window;
    a.power = power;
    a.M = sig->num_ants;
    a.F = cfg->num_bins;
    a.L = plan.log2F;
    a.H = cfg->hop;
    a.S = (int)plan.S;
    a.teams = plan.teams;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.units = plan.units;
    a.rounds = plan.rounds;
    GAT_HIP(c, launch_spectrum(a, plan, sig->layout, c->stream));
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)plan.grid;
    c->last.threads = kSpecThreads;
    c->last.splits = 1; // a (block, antenna) pair is never split
    c->last.ant_tile = 1;
    c->last.vec = plan.aligned ? layout_vec_samples(sig->layout) : 1;
    c->last.lds_bytes = spec_lds_bytes(plan.R);
    c->last.channels_per_wg = plan.teams; // (block, antenna) pairs a workgroup transforms side by side
    return GAT_OK;
}

GAT_API int32_t gat_sample_spectrum_host(const gat_signal_desc *sig, int32_t B, const float *window, const gat_spectrum_config *cfg, float *power)
{
    SpecPlan plan{};
    const Refusal r = spec_plan(sig, B, window, cfg, power, 1, &plan);
    if (r.code != GAT_OK) return r.code;
    spec_host_run(sig, B, window, cfg->num_bins, cfg->hop, power);
    return GAT_OK;
}
