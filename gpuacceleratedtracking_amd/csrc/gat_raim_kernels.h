// gat_raim_kernels.h -- what the fix integrity's kernel (gat_raim.hip) and its host side (gat_raim_api.cpp) share: the kernel's
// arguments and the launcher.  The geometry is gat_raim_plan.h, the arithmetic gat_fix.h and gat_raim.h.
#pragma once

#include "gat_fix_kernels.h"
#include "gat_raim.h"
#include "gat_raim_plan.h"

namespace gat {

// One gat_position_fix_raim call: the fix's arguments, integrity [E], trial [E][K] (null: not asked for) and the raim configuration.
struct RaimArgs {
    FixArgs fix;
    gat_fix_integrity *integrity;
    double *trial;
    int max_exclude, trial_iter;
    double threshold[kRaimThresholds];
};

// enqueues the kernel of `grid` workgroups (FixPlan::groups) on `st`
hipError_t launch_raim(const RaimArgs &a, long long grid, hipStream_t st);

} // namespace gat
