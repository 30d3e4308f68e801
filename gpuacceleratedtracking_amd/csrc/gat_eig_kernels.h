// gat_eig_kernels.h -- what the subspace kernels (gat_eig.hip) and their host side (gat_eig_api.cpp) share: the kernels' arguments
// and the launchers.  The geometry and the units' decoding are gat_eig_plan.h, the arithmetic gat_eig.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_eig.h"
#include "gat_eig_plan.h"

namespace gat {

// One gat_accumulator_covariance call.  part_re / part_im: the chunk sums in the context's scratch (split plans only).
struct AccCovArgs {
    const float *acc_re, *acc_im;
    long long acc_block_stride; // 0 with one block
    double *part_re, *part_im;
    double *cov_re, *cov_im;
    int B, K, L, M, tap, bpe, E, C, T;
};

// One gat_hermitian_eig call: the plan travels with it (the LDS carve-up is the plan's)
struct EigArgs {
    const void *a_re, *a_im;
    double *eigenvalues, *vec_re, *vec_im;
    int32_t *status;
    EigPlan p;
};

// Each launcher enqueues one kernel on `st`: the covariance's of p.g_chunk (then p.g_reduce) workgroups of kCovThreads threads with
// p.lds_bytes of LDS, the eigensolver's of p.g workgroups of p.threads threads with p.lds_bytes.
hipError_t launch_acc_cov_direct(const AccCovArgs &a, const AccCovPlan &p, hipStream_t st);
hipError_t launch_acc_cov_chunks(const AccCovArgs &a, const AccCovPlan &p, hipStream_t st);
hipError_t launch_acc_cov_reduce(const AccCovArgs &a, const AccCovPlan &p, hipStream_t st);
hipError_t launch_hermitian_eig(const EigArgs &a, hipStream_t st);

} // namespace gat
