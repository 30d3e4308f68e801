// gat_atm_kernels.h -- what the range corrections' kernel (gat_atm.hip) and its host side (gat_atm_api.cpp) share: the kernel's
// arguments and the launcher.  The geometry is gat_atm_plan.h, the arithmetic gat_atm.h on top of gat_fix.h and gat_vel.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_atm.h"
#include "gat_atm_plan.h"

namespace gat {

// One gat_range_corrections call.  eph [K]; tx_ms, tx_frac [E][K]; rx_ms, rx_frac, fixes [E]; zenith [E][2] (null: the config's);
// tx_frac_out [E][K]; delay [E][K][2], geom [E][K][3], ch_status [E][K], ep_status [E]: null where not asked for.
struct AtmArgs {
    const gat_ephemeris *eph;
    const int32_t *tx_ms;
    const double *tx_frac;
    const int32_t *rx_ms;
    const double *rx_frac;
    const gat_fix *fixes;
    const double *zenith;
    double *tx_frac_out, *delay, *geom;
    uint8_t *ch_status;
    int32_t *ep_status;
    int K;
    long long cells;
    AtmParams prm;
};

// enqueues the kernel of `grid` workgroups (AtmPlan::groups) on `st`
hipError_t launch_atm(const AtmArgs &a, long long grid, hipStream_t st);

} // namespace gat
