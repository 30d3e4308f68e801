// gat_acq_kernels.h -- what the acquisition kernels (gat_acq.hip) and their host side (gat_acq_api.cpp) share: the grid
// kernel's arguments and the launchers.  The geometry is the plan's (gat_acq_plan.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_acq_plan.h" // the grid's tile constants; kAcqMaxCodeStep (gat_acq_check.h)

namespace gat {

struct AcqArgs {
    const void *re, *im;
    int M, B;
    long long N, ant_stride, block_stride;
    const int8_t *codes;
    int code_row_stride, Lc;
    const int *prns; // [P] code-table columns
    int P, D, J, s, G;
    double ratio, fs, if_hz, f_first, f_step; // ratio = fc / fs
    long long first_shift;
    float *out; // [G][P][D][J]: the power grid itself when G == 1, else the groups' slices
};

// LDS of one grid workgroup for code step s: the Doppler steps, the wiped samples and the chunk's replica window as chip pairs
inline size_t acq_grid_lds_bytes(int s)
{
    return kAcqDopTile * sizeof(double) + (size_t)kAcqDopTile * kAcqChunk * 2 * sizeof(float) +
           (size_t)(kAcqChunk + s * (kAcqCodeTile - 1)) * 2 * sizeof(float);
}

hipError_t acq_grid_allow_lds(int s);
hipError_t launch_acq_grid(const AcqArgs &a, int fmt, hipStream_t st);
hipError_t launch_acq_sum_groups(const float *part, float *power, long long cells, int G, hipStream_t st);
hipError_t launch_acq_stats(const float *power, int P, int D, int J, const gat_acq_config &cfg, double fs, long long N,
                            const int *prns, gat_acq_result *res, hipStream_t st);

} // namespace gat
