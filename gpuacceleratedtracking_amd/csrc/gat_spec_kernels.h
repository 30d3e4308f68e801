// gat_spec_kernels.h -- what the sample spectrum's kernels (gat_spec.hip) and their host side (gat_spec_api.cpp) share: the
// kernels' arguments and the launcher.  The geometry and the work split are gat_spec_plan.h, the arithmetic gat_spec.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_spec.h"
#include "gat_spec_plan.h"

namespace gat {

// One gat_sample_spectrum call.  Input element (n, m, b) is sample n + m * ant_stride + b * block_stride of the signal's planes,
// output element (f, m, b) float f + (b * M + m) * F of power.
struct SpecArgs {
    const void *re, *im;
    const float *window;
    float *power;
    int M, F, L, H, S, teams; // L = log2 F; teams = 256 / (F / R) of plan.R
    long long ant_stride, block_stride, units, rounds;
};
// plan from spec_plan; plan.aligned: every block of every antenna on a 16-byte boundary and H a multiple of a load's samples
hipError_t launch_spectrum(const SpecArgs &a, const SpecPlan &plan, int fmt, hipStream_t st);
// LDS of a workgroup: the points of its teams and the twiddles
constexpr int spec_lds_bytes(int R) { return (int)sizeof(float2) * (kSpecThreads * R + kSpecThreads * R / 2); }

} // namespace gat
