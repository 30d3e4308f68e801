// gat_acq_fft_kernels.h -- what the FFT acquisition kernels (gat_acq_fft.hip) and their host side (gat_acq_fft_api.cpp) share: the
// arguments and the launchers.  The geometry is the plan's (gat_acq_fft_plan.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_acq_fft_plan.h"

namespace gat {

constexpr int kAcqFftThreads = 256;

struct AcqFftArgs {
    const void *re, *im;
    int M, B;
    long long N, ant_stride, block_stride;
    const int8_t *codes;
    int code_row_stride, Lc;
    const int *prns; // [P] code-table columns
    int P, D, J, s;
    double ratio, fs, if_hz, f_first, f_step; // ratio = fc / fs
    long long first_shift;
    // the plan
    int L, L1, L2, tiles, G, Db, Gu, Bb;
    long long Jseg, units, cells;
    float scale;  // 2^(-2 L)
    float2 *tw;   // [F / 2]
    float2 *C;    // [P][Bb][G][F]
    float2 *W;    // [Ub][Db][F]
    float2 *Y;    // [Gu][P][Db][G][F]: the product's first pass (two passes only)
    float *out;   // [Gu][P][D][J]: the power grid itself when Gu == 1, else the groups' slices
    // the batch and the step of this launch
    int i0, dn;   // Doppler bins [i0, i0 + dn)
    int u0, un;   // units [u0, u0 + un): the W slots
    int b0, bn;   // blocks [b0, b0 + bn): the C slots
    int us;       // the step's first unit (a multiple of Gu): group k correlates unit us + k
};

hipError_t launch_acq_fft_twiddles(const AcqFftArgs &a, hipStream_t st);
hipError_t launch_acq_fft_replica(const AcqFftArgs &a, hipStream_t st);           // C of P x bn x G
hipError_t launch_acq_fft_signal(const AcqFftArgs &a, int fmt, hipStream_t st);   // W of un x dn
hipError_t launch_acq_fft_correlate(const AcqFftArgs &a, hipStream_t st);         // one step: Gu x P x dn x G products into the grid

} // namespace gat
