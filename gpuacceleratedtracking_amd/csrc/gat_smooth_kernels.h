// gat_smooth_kernels.h -- what the carrier smoothing's kernels (gat_smooth.hip) and their host side (gat_smooth_api.cpp) share: the
// kernels' arguments and the launcher.  The geometry and the scratch layout are gat_smooth_plan.h, the arithmetic gat_smooth.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_smooth.h"
#include "gat_smooth_plan.h"

namespace gat {

// One gat_smooth_observables call.  in, out: the call's arrays, null where not given / not asked for.  The rest is the context's
// scratch as SmPlan lays it out.
struct SmArgs {
    SmIn in;
    SmOut out;
    SmRule rule;
    int E, K, chunks, lanes, rows, run;
    long long cells;
    SmSeg *totals; // [chunks][K]: the chunks' segments, after the channel kernel their exclusive prefixes
    SmSeg *runs;   // [chunks][kSmThreads]
    uint64_t *C;   // [E][K]
    uint64_t *SS;  // [E][K]
    int32_t *arc;  // [E][K]: a(e), -1 where not measured
};

// enqueues the four kernels of a planned call on `st`: chunk totals, channel scan, emit, output
hipError_t launch_smooth(const SmArgs &a, const SmPlan &p, hipStream_t st);

} // namespace gat
