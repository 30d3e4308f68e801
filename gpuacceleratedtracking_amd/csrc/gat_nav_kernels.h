// gat_nav_kernels.h -- what the navigation data layer's kernels (gat_nav.hip) and their host side (gat_nav_api.cpp) share: the
// kernels' arguments and the launchers.  The geometry and the units' decoding are gat_nav_plan.h, the arithmetic gat_nav.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_nav.h"
#include "gat_nav_plan.h"

namespace gat {

// One gat_nav_decode call.  q [K][cap], surv [K][2][bit_cap] and scores [K][C]: scratch; decoded [K][P][bit_cap] and chan [K]: the
// caller's buffers or scratch; frames and path_metric: the caller's outputs, null where not asked for; mon: null or the monitor's
// records, read on the device.
struct NavArgs {
    const double *sym_re;
    const gat_monitor_channel *mon;
    int8_t *q;
    unsigned long long *surv;
    uint8_t *decoded;
    int32_t *scores;
    gat_nav_channel *chan;
    gat_nav_frame *frames;
    int32_t *path_metric;
    int format, K, cap, P, bit_cap, max_frames, min_frames, C;
};

// Each launcher enqueues one kernel of `grid` workgroups (NavPlan::g_*, > 0) on `st`.
hipError_t launch_nav_slice(const NavArgs &a, long long grid, hipStream_t st);
hipError_t launch_nav_quantise(const NavArgs &a, long long grid, hipStream_t st);
hipError_t launch_nav_trellis(const NavArgs &a, long long grid, hipStream_t st);
hipError_t launch_nav_score(const NavArgs &a, long long grid, hipStream_t st);
hipError_t launch_nav_pick(const NavArgs &a, long long grid, hipStream_t st);   // writes the channel records to device memory
hipError_t launch_nav_frames(const NavArgs &a, long long grid, hipStream_t st); // reads them there

} // namespace gat
