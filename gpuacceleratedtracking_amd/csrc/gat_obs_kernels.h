// gat_obs_kernels.h -- what the observables' kernels (gat_obs.hip) and their host side (gat_obs_api.cpp) share: the kernels'
// arguments and the launcher.  The geometry and the scratch layout are gat_obs_plan.h, the arithmetic gat_obs.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_obs.h"
#include "gat_obs_plan.h"

namespace gat {

// One gat_observables call.  hist [B + 1][K]; mon, nav [K]; frames [K][max_frames]; out: null where not asked for.  The rest is the
// context's scratch as ObsPlan lays it out.
struct ObsArgs {
    const gat_channel_params *hist;
    const gat_monitor_channel *mon;
    const gat_nav_channel *nav;
    const gat_nav_frame *frames;
    ObsOut out;
    ObsRule rule;
    int chunks, group, groups, lanes, rows, run;
    ObsSum *totals; // [chunks][K]: the chunks' sums, after the channel kernel their exclusive prefixes
    int32_t *bad;   // [chunks][K]
    ObsSum *runs;   // [chunks][groups][kObsThreads]
    ObsChan *chan;  // [K]
    ObsAnchor *anchor;
};

// enqueues the four kernels of a planned call on `st`: sums, channels, anchor, epochs
hipError_t launch_obs(const ObsArgs &a, const ObsPlan &p, hipStream_t st);

} // namespace gat
