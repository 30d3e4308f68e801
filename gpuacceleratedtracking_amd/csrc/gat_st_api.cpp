// gat_st_api.cpp -- host side of space-time adaptive processing (include/gat.h gat_spacetime_covariance, gat_spacetime_filter): the
// launches behind the pure plans of gat_st_plan.h, and the filter's host twin (gat_spacetime_filter_host), which runs the loop of
// gat_st.h.  The kernels are gat_st.hip; the weights' narrowing is the beamformer's (gat_beam.hip), the covariance's finishing
// kernel the spatial covariance's (gat_array.hip).
#include <algorithm>

#include "gat_beam_kernels.h"
#include "gat_ctx.h"
#include "gat_st_kernels.h"

using namespace gat;

GAT_API int32_t gat_spacetime_covariance(gat_ctx *c, const gat_signal_desc *sig, int32_t B, int32_t bpe, int32_t T, float *cov_re, float *cov_im)
{
    if (!c) return GAT_ERR_ARG;
    StCovPlan plan{};
    const Refusal r = st_cov_plan(sig, B, bpe, T, cov_re, cov_im, c->num_cus, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    if (T == 1) return gat_spatial_covariance(c, sig, B, bpe, cov_re, cov_im); // one tap: the spatial covariance, and its bits
    GAT_ENTER(c, "gat_spacetime_covariance");
    const int Q = plan.Q;
    return enqueue_estimates<CovArgs>(c, sig, plan.est, [&](CovArgs a, const EstimateLaunches &t) -> int32_t {
        a.partial = c->d_partial;
        GAT_HIP(c, launch_st_cov(a, T, sig->layout, c->stream));
        GAT_HIP(c, launch_cov_finish(c->d_partial, Q, t.en, (int)t.G, cov_re + (size_t)t.e0 * Q * Q, cov_im + (size_t)t.e0 * Q * Q, c->stream));
        return GAT_OK;
    });
}

GAT_API int32_t gat_spacetime_filter(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const double *w_re, const double *w_im, int32_t T, int32_t J,
                                     const gat_signal_desc *out)
{
    if (!c) return GAT_ERR_ARG;
    StPlan plan{};
    const Refusal r = st_filter_plan(sig, B, w_re, w_im, T, J, out, (long long)c->num_cus * 8, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    // one tap: the snapshot is the antenna vector, the rule and the bits are gat_beamform_samples', and so are its kernels
    if (T == 1) return gat_beamform_samples(c, sig, B, w_re, w_im, J, out);
    GAT_ENTER(c, "gat_spacetime_filter");
    const int M = sig->num_ants, Q = M * T;
    const int32_t rc = ensure_partial(c, beam_weight_count(J, Q, plan.beams) * sizeof(float2));
    if (rc != GAT_OK) return rc;
    float2 *w32 = reinterpret_cast<float2 *>(c->d_partial);
    StArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.out_re = static_cast<float *>(const_cast<void *>(out->re));
    a.out_im = static_cast<float *>(const_cast<void *>(out->im));
    a.M = M;
    a.T = T;
    a.J = J;
    a.tile = plan.tile;
    a.row = plan.row;
    a.N = sig->num_samples;
    a.outputs = plan.outputs;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.out_ant_stride = out->ant_stride;
    a.out_block_stride = out->block_stride;
    a.chunk = plan.chunk;
    a.chunks = plan.chunks;
    a.units = plan.units;
    GAT_HIP(c, launch_beam_weights(w_re, w_im, J, Q, plan.beams, w32, c->stream)); // the one narrowing, in tiles of plan.beams beams
    GAT_HIP(c, plan.tiled ? launch_st_tiled(a, sig->layout, w32, (int)plan.grid, c->stream)
                          : launch_st_general(a, sig->layout, w32, (int)plan.grid, c->stream));
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)plan.grid;
    c->last.threads = kStThreads;
    c->last.splits = (int32_t)plan.chunks;
    c->last.ant_tile = M;
    c->last.vec = plan.tiled ? layout_vec_samples(sig->layout) : 1;
    // the tiled kernel's samples and one pass's weights; the general kernel's weights
    c->last.lds_bytes = (int32_t)sizeof(float2) * (plan.tiled ? kStLdsSamples + GAT_MAX_ARRAY_ANTS * plan.beams : GAT_MAX_ARRAY_ANTS * plan.beams);
    return GAT_OK;
}

GAT_API int32_t gat_spacetime_filter_host(const gat_signal_desc *sig, int32_t B, const double *w_re, const double *w_im, int32_t T, int32_t J,
                                          const gat_signal_desc *out)
{
    StPlan plan{};
    const Refusal r = st_filter_plan(sig, B, w_re, w_im, T, J, out, 1, &plan);
    if (r.code != GAT_OK) return r.code;
    st_host_run(sig, B, w_re, w_im, T, J, out);
    return GAT_OK;
}
