// gat_vel_kernels.h -- what the velocity fix's kernel (gat_vel.hip) and its host side (gat_vel_api.cpp) share: the kernel's
// arguments and the launcher.  The geometry is gat_vel_plan.h, the arithmetic gat_vel.h on top of gat_fix.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_vel.h"
#include "gat_vel_plan.h"

namespace gat {

// One gat_velocity_fix call.  eph [K]; tx_ms, tx_frac, doppler [E][K]; fixes [E]; used_in, w [E][K] (null: every channel, 1);
// vel [E]; sat_vel [E][K][4], resid [E][K]: null where not asked for.
struct VelArgs {
    const gat_ephemeris *eph;
    const int32_t *tx_ms;
    const double *tx_frac;
    const double *doppler;
    const gat_fix *fixes;
    const uint8_t *used_in;
    const double *w;
    gat_velocity *vel;
    double *sat_vel, *resid;
    int E, K;
    double lambda;
};

// enqueues the kernel of `grid` workgroups (VelPlan::groups) on `st`
hipError_t launch_vel(const VelArgs &a, long long grid, hipStream_t st);

} // namespace gat
