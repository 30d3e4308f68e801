// gat_array_api.cpp -- host side of the antenna-array entry points (include/gat.h gat_spatial_covariance, gat_array_weights,
// gat_beamform, gat_tracking_update_weighted, gat_tracking_run_weighted): validation and the launch sequences; the covariance's
// refusals, kernel choice and work split are the pure plan of gat_array_plan.h.  The host-only twins (gat_array_weights_host,
// gat_tracking_update_host_weighted) live in gat_codes.cpp.
#include <cmath>
#include <cstring>

#include "gat_array_kernels.h"
#include "gat_ctx.h"

using namespace gat;

GAT_API int32_t gat_spatial_covariance(gat_ctx *c, const gat_signal_desc *sig, int32_t B, int32_t bpe, float *cov_re, float *cov_im)
{
    if (!c) return GAT_ERR_ARG;
    CovPlan plan{};
    const Refusal r = cov_plan(sig, B, bpe, cov_re, cov_im, c->num_cus, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_spatial_covariance");
    const int M = sig->num_ants, layout = sig->layout;
    return enqueue_estimates<CovArgs>(c, sig, plan.est, [&](CovArgs a, const EstimateLaunches &t) -> int32_t {
        a.partial = c->d_partial;
        GAT_HIP(c, plan.vec ? launch_cov_small(a, layout, c->stream) : launch_cov_tiled(a, layout, c->stream));
        GAT_HIP(c, launch_cov_finish(c->d_partial, M, t.en, (int)t.G, cov_re + (size_t)t.e0 * M * M, cov_im + (size_t)t.e0 * M * M, c->stream));
        return GAT_OK;
    });
}

GAT_API int32_t gat_array_weights(gat_ctx *c, const float *cov_re, const float *cov_im, int32_t M, const double *steer_re, const double *steer_im,
                                  int32_t K, int32_t mode, double loading, double *w_re, double *w_im)
{
    if (!c) return GAT_ERR_ARG;
    if (!w_re || !w_im || K < 1 || M < 1) return fail(c, GAT_ERR_ARG, "null output or empty sizes");
    if (mode != GAT_BF_CONVENTIONAL && mode != GAT_BF_MVDR && mode != GAT_BF_POWER_INVERSION) return fail(c, GAT_ERR_ARG, "bad mode");
    if (mode != GAT_BF_POWER_INVERSION && (!steer_re || !steer_im)) return fail(c, GAT_ERR_ARG, "this mode needs steering vectors");
    if (mode != GAT_BF_CONVENTIONAL && (!cov_re || !cov_im)) return fail(c, GAT_ERR_ARG, "this mode needs a covariance");
    if (!(loading >= 0.0) || !std::isfinite(loading)) return fail(c, GAT_ERR_ARG, "loading must be finite and not negative");
    if (M > GAT_MAX_ARRAY_ANTS) return fail(c, GAT_ERR_RANGE, "more than 64 antennas");
    if (K > 65535) return fail(c, GAT_ERR_RANGE, "too many channels for one call");
    GAT_ENTER(c, "gat_array_weights");
    const int32_t rc = ensure_partial(c, ((size_t)2 * M * M + 1) * sizeof(double));
    if (rc != GAT_OK) return rc;
    GAT_HIP(c, array_weights_allow_lds());
    GAT_HIP(c, launch_array_weights(cov_re, cov_im, M, steer_re, steer_im, K, mode, loading, reinterpret_cast<double *>(c->d_partial), w_re, w_im,
                                    c->stream));
    return GAT_OK;
}

GAT_API int32_t gat_beamform(gat_ctx *c, const float *acc_re, const float *acc_im, int32_t B, int32_t K, int32_t L, int32_t M, const double *w_re,
                             const double *w_im, float *out_re, float *out_im)
{
    if (!c) return GAT_ERR_ARG;
    if (!acc_re || !acc_im || !w_re || !w_im || !out_re || !out_im) return fail(c, GAT_ERR_ARG, "null argument");
    if (B < 1 || K < 1 || L < 1 || M < 1) return fail(c, GAT_ERR_ARG, "sizes must be positive");
    const long long rows = (long long)B * K * L;
    if (rows > ((long long)1 << 38)) return fail(c, GAT_ERR_RANGE, "too many accumulators for one call");
    GAT_ENTER(c, "gat_beamform");
    GAT_HIP(c, launch_beamform(acc_re, acc_im, rows, K, L, M, w_re, w_im, out_re, out_im, c->stream));
    return GAT_OK;
}

GAT_API int32_t gat_tracking_update_weighted(gat_ctx *c, const float *acc_re, const float *acc_im, int32_t K, int32_t M, const gat_loop_config *cfg,
                                             gat_loop_state *state, const gat_channel_params *cur, gat_channel_params *next, const double *w_re,
                                             const double *w_im)
{
    if (!w_re && !w_im) return gat_tracking_update(c, acc_re, acc_im, K, M, cfg, state, cur, next); // today's path, today's bits
    if (!c || !acc_re || !acc_im || !cfg || !state || !cur || !next || !w_re || !w_im) return fail(c, GAT_ERR_ARG, "null argument");
    if (K < 1 || M < 1) return fail(c, GAT_ERR_ARG, "sizes must be positive");
    const int32_t rc = check_loop_config(c, cfg);
    if (rc != GAT_OK) return rc;
    GAT_ENTER(c, "gat_tracking_update_weighted");
    GAT_HIP(c, launch_tracking_update_weighted(acc_re, acc_im, K, M, *cfg, state, cur, next, w_re, w_im, c->stream));
    return GAT_OK;
}

GAT_API int32_t gat_tracking_run_weighted(gat_ctx *c, const gat_signal_desc *sig, int32_t num_blocks, int32_t K, int32_t L, const int32_t *shifts,
                                          double fs, const gat_loop_config *cfg, gat_loop_state *state, gat_channel_params *params_a,
                                          gat_channel_params *params_b, float *acc_re, float *acc_im, int64_t acc_block_stride, uint32_t flags,
                                          int32_t *current_is_b, const double *w_re, const double *w_im)
{
    if (!w_re && !w_im)
        return gat_tracking_run(c, sig, num_blocks, K, L, shifts, fs, cfg, state, params_a, params_b, acc_re, acc_im, acc_block_stride, flags,
                                current_is_b);
    if (!w_re || !w_im) return fail(c, GAT_ERR_ARG, "null argument"); // (the other null checks are tracking_run_shared's)
    return tracking_run_shared(c, sig, num_blocks, K, L, shifts, fs, cfg, state, params_a, params_b, acc_re, acc_im, acc_block_stride, flags,
                               current_is_b, w_re, w_im);
}
