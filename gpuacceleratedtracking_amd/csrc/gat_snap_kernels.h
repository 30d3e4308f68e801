// gat_snap_kernels.h -- what the snapshot fix's kernel (gat_snap.hip) and its host side (gat_snap_api.cpp) share: the kernel's
// arguments and the launcher.  The geometry is gat_snap_plan.h, the arithmetic gat_snap.h on top of gat_fix.h and gat_vel.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_snap.h"
#include "gat_snap_plan.h"

namespace gat {

// One gat_snapshot_fix call.  eph [K]; code_frac, w [E][K] (w null: 1); rx_ms, rx_frac [E]; prior [E][3] (null: init_xyz); fixes
// [E]; tx_ms, n_ms, resid, sin_el, used [E][K], rx_ms_out [E]: null where not asked for.
struct SnapArgs {
    const gat_ephemeris *eph;
    const double *code_frac;
    const int32_t *rx_ms;
    const double *rx_frac;
    const double *prior, *w;
    gat_snap_fix *fixes;
    int32_t *tx_ms, *rx_ms_out, *n_ms;
    double *resid, *sin_el;
    uint8_t *used;
    int E, K, max_iter;
    double tol_m, mask_sin, init_xyz[3], margin;
};

// enqueues the kernel of `grid` workgroups (SnapPlan::groups) on `st`
hipError_t launch_snap(const SnapArgs &a, long long grid, hipStream_t st);

} // namespace gat
