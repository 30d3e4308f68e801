// gat_array_kernels.h -- what the array kernels (gat_array.hip) and their host side (gat_array_api.cpp) share: the kernels'
// arguments and the launchers.  The covariance kernels' geometry and the work split are gat_array_plan.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_array_plan.h"

namespace gat {

// One covariance call.  Work units are (block, segment of seg_len samples): estimate e owns blocks [e * bpe, min(B, (e+1) * bpe))
// and G workgroups (workgroup e * G + g of the grid); workgroup g of e takes its units g, g + G, ... and writes its sums to slice
// (e * G + g) of `partial` ([2][M][M] floats, upper triangle only).
struct CovArgs {
    const void *re, *im;
    int M, B, bpe, E, G, splits;
    long long N, ant_stride, block_stride, seg_len;
    float *partial;
};

hipError_t launch_cov_small(const CovArgs &a, int fmt, hipStream_t st);  // M <= 8, 16-byte loads
hipError_t launch_cov_tiled(const CovArgs &a, int fmt, hipStream_t st);  // any M <= 64, any alignment
hipError_t launch_cov_finish(const float *partial, int M, int E, int G, float *cov_re, float *cov_im, hipStream_t st);
hipError_t array_weights_allow_lds(); // 64 antennas need more than 64 KB of LDS for the factor's two FP64 planes
// l_re | l_im | ok: scratch of 2 * M * M doubles and one int the factor kernel writes and the solve kernel reads
hipError_t launch_array_weights(const float *cov_re, const float *cov_im, int M, const double *steer_re, const double *steer_im, int K,
                                int mode, double loading, double *scratch, double *w_re, double *w_im, hipStream_t st);
hipError_t launch_beamform(const float *acc_re, const float *acc_im, long long rows, int K, int L, int M, const double *w_re,
                           const double *w_im, float *out_re, float *out_im, hipStream_t st);
hipError_t launch_tracking_update_weighted(const float *acc_re, const float *acc_im, int K, int M, const gat_loop_config &cfg,
                                           gat_loop_state *state, const gat_channel_params *cur, gat_channel_params *next,
                                           const double *w_re, const double *w_im, hipStream_t st);

} // namespace gat
