// gat_mon_kernels.h -- what the tracking monitor's kernels (gat_mon.hip) and their host side (gat_mon_api.cpp) share: the kernels'
// arguments and the launchers.  The geometry and the units' decoding are gat_mon_plan.h, the arithmetic gat_mon.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_mon.h"
#include "gat_mon_plan.h"

namespace gat {

// One gat_track_monitor call.  pr / pi: the prompt series [K][B] (the caller's buffers or scratch); terms [K][J][Pd], energy
// [K][Pd] and chan [K]: the caller's buffers or scratch; the rest are the caller's outputs, null where not asked for.
struct MonArgs {
    const float *acc_re, *acc_im;
    long long acc_block_stride;
    const double *w_re, *w_im;
    double *pr, *pi, *terms, *energy;
    gat_monitor_channel *chan;
    gat_monitor_window *windows;
    double *sym_re, *sym_im, *sym_wbp;
    int B, K, M, L, prompt, W, Pd, forced;
    long long first_block, NW, J, cap;
    int8_t overlay[GAT_MAX_SYMBOL_BLOCKS];
};

// Each launcher enqueues one kernel of `grid` workgroups of kMonThreads threads (MonPlan::g_*, > 0) on `st`.
hipError_t launch_mon_prompts(const MonArgs &a, long long grid, hipStream_t st);
hipError_t launch_mon_windows(const MonArgs &a, long long grid, hipStream_t st);
hipError_t launch_mon_terms(const MonArgs &a, long long grid, hipStream_t st);
hipError_t launch_mon_energies(const MonArgs &a, long long grid, hipStream_t st); // J == 0: writes E = 0
hipError_t launch_mon_pick(const MonArgs &a, long long grid, hipStream_t st);
hipError_t launch_mon_symbols(const MonArgs &a, long long grid, hipStream_t st);  // reads the channel records on the device

} // namespace gat
