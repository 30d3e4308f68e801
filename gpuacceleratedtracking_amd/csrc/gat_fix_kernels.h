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

// the arguments of a planned call: the plan's sizes and rule, the call's pointers (gat_fix_api.cpp, gat_raim_api.cpp)
inline FixArgs fix_args(const FixPlan &p, const gat_ephemeris *eph, const int32_t *tx_ms, const double *tx_frac, const int32_t *rx_ms,
                        const double *rx_frac, const double *weights, gat_fix *fixes, double *sat, double *resid, double *sin_el, uint8_t *used)
{
    FixArgs a{};
    a.eph = eph, a.tx_ms = tx_ms, a.tx_frac = tx_frac, a.rx_ms = rx_ms, a.rx_frac = rx_frac, a.w = weights;
    a.fixes = fixes, a.sat = sat, a.resid = resid, a.sin_el = sin_el, a.used = used;
    a.E = p.E, a.K = p.K, a.max_iter = p.max_iter, a.tol_m = p.tol_m, a.mask_sin = p.mask_sin;
    for (int i = 0; i < 3; ++i) a.init_xyz[i] = p.init_xyz[i];
    return a;
}

// enqueues the kernel of `grid` workgroups (FixPlan::groups) on `st`
hipError_t launch_fix(const FixArgs &a, long long grid, hipStream_t st);

} // namespace gat
