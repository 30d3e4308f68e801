// gat_beam_api.cpp -- host side of gat_beamform_samples (include/gat.h): the launches behind the pure plan of gat_beam_plan.h.
// The kernels are gat_beam.hip.
#include "gat_beam_kernels.h"
#include "gat_ctx.h"

using namespace gat;

GAT_API int32_t gat_beamform_samples(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const double *w_re, const double *w_im, int32_t J,
                                     const gat_signal_desc *out)
{
    if (!c) return GAT_ERR_ARG;
    BeamPlan plan{};
    const Refusal r = beam_plan(sig, B, w_re, w_im, J, out, (long long)c->num_cus * 8, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_beamform_samples");
    const int M = sig->num_ants, T = beam_tile(plan.stream, J);
    const int32_t rc = ensure_partial(c, beam_weight_count(J, M, T) * sizeof(float2));
    if (rc != GAT_OK) return rc;
    float2 *w32 = reinterpret_cast<float2 *>(c->d_partial);
    BeamArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.out_re = static_cast<float *>(const_cast<void *>(out->re));
    a.out_im = static_cast<float *>(const_cast<void *>(out->im));
    a.M = M;
    a.B = B;
    a.J = J;
    a.chunks = (int)plan.chunks;
    a.N = sig->num_samples;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.out_ant_stride = out->ant_stride;
    a.out_block_stride = out->block_stride;
    a.chunk = plan.chunk;
    GAT_HIP(c, launch_beam_weights(w_re, w_im, J, M, T, w32, c->stream));
    GAT_HIP(c, plan.stream ? launch_beam_stream(a, sig->layout, w32, (int)plan.grid, c->stream)
                           : launch_beam_general(a, sig->layout, w32, (int)plan.grid, c->stream));
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)plan.grid;
    c->last.threads = kBeamThreads;
    c->last.splits = (int32_t)plan.chunks;
    c->last.ant_tile = M;
    c->last.vec = plan.stream ? 4 : 1;
    // the weights in LDS: the general kernel's [64][T] float2; the streaming kernel's [M][T] when T > 1 (one beam: scalar loads, no LDS)
    c->last.lds_bytes = (int32_t)sizeof(float2) * (plan.stream ? (T > 1 ? M * T : 0) : GAT_MAX_ARRAY_ANTS * T);
    return GAT_OK;
}
