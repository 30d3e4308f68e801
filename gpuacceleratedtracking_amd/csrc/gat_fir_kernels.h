// gat_fir_kernels.h -- what the sample filter's kernels (gat_fir.hip) and their host side (gat_fir_api.cpp) share: the kernels'
// arguments and the launchers.  The geometry and the work split are gat_fir_plan.h, the arithmetic gat_fir.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_fir.h"
#include "gat_fir_plan.h"

namespace gat {

// One gat_filter_samples call.  Input element (n, m, b) is sample n + m * ant_stride + b * block_stride of the signal's planes,
// output element (q, m, b) float q + m * out_ant_stride + b * out_block_stride of the output's.
struct FirArgs {
    const void *re, *im;
    float *out_re, *out_im;
    const float *taps_re, *taps_im;
    int M, T, D, tile, row;
    long long N, Q, ant_stride, block_stride, out_ant_stride, out_block_stride, chunk, chunks, units;
    FirNco nco;
};
// every block of every antenna on a 16-byte boundary on both sides; a.tile, a.row from fir_plan
hipError_t launch_fir_tiled(const FirArgs &a, int fmt_in, int fmt_out, int grid, hipStream_t st);
// any alignment and strides
hipError_t launch_fir_general(const FirArgs &a, int fmt_in, int fmt_out, int grid, hipStream_t st);

} // namespace gat
