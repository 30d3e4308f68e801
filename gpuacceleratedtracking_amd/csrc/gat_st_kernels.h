// gat_st_kernels.h -- what the space-time kernels (gat_st.hip) and their host side (gat_st_api.cpp) share: the kernels' arguments
// and the launchers.  The geometry and the work split are gat_st_plan.h, the arithmetic gat_st.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_array_kernels.h" // CovArgs, launch_cov_finish: the covariance's slices and their finishing kernel are the spatial one's
#include "gat_st.h"
#include "gat_st_plan.h"

namespace gat {

// One gat_spacetime_filter call.  Input element (n, m, b) is sample n + m * ant_stride + b * block_stride of the signal's planes;
// output element (n', j, b) is float n' + j * out_ant_stride + b * out_block_stride of out_re / out_im (planar), or that float2 of
// out_re (out_im == nullptr: interleaved).  Units, chunks, tile and row: StPlan.
struct StArgs {
    const void *re, *im;
    float *out_re, *out_im;
    int M, T, J, tile, row;
    long long N, outputs, ant_stride, block_stride, out_ant_stride, out_block_stride, chunk, chunks, units;
};

// w32: the weights narrowed by launch_beam_weights (gat_beam_kernels.h) with Q for M and the plan's beam tile JT:
// w32[((j / JT) * Q + q) * JT + j % JT]
// M <= kStTiledMaxAnts, every block of every antenna and beam on a 16-byte boundary; a.tile, a.row from st_filter_plan
hipError_t launch_st_tiled(const StArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st);
// any M * T <= 64, any alignment and strides; a.chunk a multiple of kStThreads
hipError_t launch_st_general(const StArgs &a, int fmt, const float2 *w32, int grid, hipStream_t st);

// The space-time covariance's partial sums: CovArgs with N the number of SNAPSHOTS of a block (seg_len, splits over them) and
// slices of [2][Q][Q] floats, Q = a.M * T, which launch_cov_finish(partial, Q, ...) ends.
hipError_t launch_st_cov(const CovArgs &a, int T, int fmt, hipStream_t st);

} // namespace gat
