// gat_fix_kernels.h -- what the position fix's kernel (gat_fix.hip) and its host side (gat_fix_api.cpp) share: the kernel's
// arguments and the launcher.  The geometry is gat_fix_plan.h, the arithmetic gat_fix.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_fix.h"
#include "gat_fix_plan.h"

namespace gat {

// One gat_position_fix call.  eph [K]; tx_ms, tx_frac, w [E][K] (w null: 1); rx_ms, rx_frac [E]; fixes [E]; sat [E][K][4], resid,
// sin_el, used [E][K]: null where not asked for.
struct FixArgs {
    const gat_ephemeris *eph;
    const int32_t *tx_ms;
    const double *tx_frac;
    const int32_t *rx_ms;
    const double *rx_frac;
    const double *w;
    gat_fix *fixes;
    double *sat, *resid, *sin_el;
    uint8_t *used;
    int E, K, max_iter;
    double tol_m, mask_sin, init_xyz[3];
};

// enqueues the kernel of `grid` workgroups (FixPlan::groups) on `st`
hipError_t launch_fix(const FixArgs &a, long long grid, hipStream_t st);

} // namespace gat
