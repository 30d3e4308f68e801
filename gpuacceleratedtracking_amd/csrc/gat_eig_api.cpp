// gat_eig_api.cpp -- host side of the subspace layer (include/gat.h gat_accumulator_covariance, gat_hermitian_eig, gat_subspace_plan
// and the two host twins): the launch sequences behind the pure plans of gat_eig_plan.h -- {chunk sums; their sum} or the one
// kernel that walks its chunks, and one workgroup per matrix of the eigensolver --, and the host twins (the loops are
// acc_cov_host_run and eig_host_one, gat_eig_plan.h).
#include "gat_ctx.h"
#include "gat_eig_kernels.h"

using namespace gat;

GAT_API int32_t gat_subspace_plan(int64_t stride, int32_t B, int32_t K, int32_t L, int32_t M, int32_t tap, int32_t bpe, int32_t n, int32_t Q, int32_t R,
                                  gat_subspace_plan_info *out)
{
    if (!out || out->struct_size < sizeof(gat_subspace_plan_info)) return GAT_ERR_ARG;
    if (B == 0 && n == 0) return GAT_ERR_ARG;
    const void *const given = out; // a stand-in for the pointers the plans only compare with null
    AccCovPlan cp{};
    EigPlan ep{};
    if (B != 0) {
        const Refusal r = acc_cov_plan(AccCovCall{given, given, stride, B, K, L, M, tap, bpe, given, given}, &cp);
        if (r.code != GAT_OK) return r.code;
    }
    if (n != 0) {
        const Refusal r = eig_plan(EigCall{given, given, n, Q, R, 0u, given, R > 0 ? given : nullptr, R > 0 ? given : nullptr, given}, &ep);
        if (r.code != GAT_OK) return r.code;
    }
    subspace_report(B != 0 ? &cp : nullptr, n != 0 ? &ep : nullptr, out);
    return GAT_OK;
}

GAT_API int32_t gat_accumulator_covariance(gat_ctx *c, const float *acc_re, const float *acc_im, int64_t stride, int32_t B, int32_t K, int32_t L,
                                           int32_t M, int32_t tap, int32_t bpe, double *cov_re, double *cov_im)
{
    if (!c) return GAT_ERR_ARG;
    AccCovPlan p{};
    const Refusal r = acc_cov_plan(AccCovCall{acc_re, acc_im, stride, B, K, L, M, tap, bpe, cov_re, cov_im}, &p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_accumulator_covariance");
    if (p.bytes > 0) {
        const int32_t rc = ensure_partial(c, p.bytes);
        if (rc != GAT_OK) return rc;
    }
    char *scratch = reinterpret_cast<char *>(c->d_partial);
    AccCovArgs a{};
    a.acc_re = acc_re, a.acc_im = acc_im, a.acc_block_stride = B > 1 ? stride : 0;
    a.part_re = p.split ? reinterpret_cast<double *>(scratch + p.off_re) : nullptr;
    a.part_im = p.split ? reinterpret_cast<double *>(scratch + p.off_im) : nullptr;
    a.cov_re = cov_re, a.cov_im = cov_im;
    a.B = p.B, a.K = p.K, a.L = p.L, a.M = p.M, a.tap = p.tap, a.bpe = p.bpe, a.E = p.E, a.C = p.C, a.T = p.T;
    if (p.split) {
        GAT_HIP(c, launch_acc_cov_chunks(a, p, c->stream));
        GAT_HIP(c, launch_acc_cov_reduce(a, p, c->stream));
    } else
        GAT_HIP(c, launch_acc_cov_direct(a, p, c->stream));
    set_last_launch(c, p.g_chunk, kCovThreads, p.split ? p.C : 1, p.M, p.lds_bytes);
    return GAT_OK;
}

GAT_API int32_t gat_accumulator_covariance_host(const float *acc_re, const float *acc_im, int64_t stride, int32_t B, int32_t K, int32_t L, int32_t M,
                                                int32_t tap, int32_t bpe, double *cov_re, double *cov_im)
{
    AccCovPlan p{};
    const Refusal r = acc_cov_plan(AccCovCall{acc_re, acc_im, stride, B, K, L, M, tap, bpe, cov_re, cov_im}, &p);
    if (r.code != GAT_OK) return r.code;
    acc_cov_host_run(p, acc_re, acc_im, stride, cov_re, cov_im);
    return GAT_OK;
}

GAT_API int32_t gat_hermitian_eig(gat_ctx *c, const void *a_re, const void *a_im, int32_t n, int32_t Q, int32_t R, uint32_t flags, double *eigenvalues,
                                  double *vec_re, double *vec_im, int32_t *status)
{
    if (!c) return GAT_ERR_ARG;
    EigArgs a{};
    const Refusal r = eig_plan(EigCall{a_re, a_im, n, Q, R, flags, eigenvalues, vec_re, vec_im, status}, &a.p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_hermitian_eig");
    a.a_re = a_re, a.a_im = a_im, a.eigenvalues = eigenvalues, a.vec_re = vec_re, a.vec_im = vec_im, a.status = status;
    GAT_HIP(c, launch_hermitian_eig(a, c->stream));
    set_last_launch(c, a.p.g, a.p.threads, 1, a.p.Q, a.p.lds_bytes);
    return GAT_OK;
}

GAT_API int32_t gat_hermitian_eig_host(const void *a_re, const void *a_im, int32_t n, int32_t Q, int32_t R, uint32_t flags, double *eigenvalues,
                                       double *vec_re, double *vec_im, int32_t *status)
{
    EigPlan p{};
    const Refusal r = eig_plan(EigCall{a_re, a_im, n, Q, R, flags, eigenvalues, vec_re, vec_im, status}, &p);
    if (r.code != GAT_OK) return r.code;
    for (int mat = 0; mat < n; ++mat) eig_host_one(p, a_re, a_im, mat, eigenvalues, vec_re, vec_im, status);
    return GAT_OK;
}
