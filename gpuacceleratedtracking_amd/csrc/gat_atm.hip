// gat_atm.hip -- the range corrections' kernel (include/gat.h gat_range_corrections) for gfx950.  The arithmetic is gat_atm.h on top
// of gat_fix.h and gat_vel.h (the host twin runs the same text), the geometry gat_atm_plan.h.
//
// Every (epoch, channel) is independent: nothing is summed across channels, so there is no LDS, no barrier and no atomic.  Thread
// t = e K + k holds channel k of epoch e, so a wave's loads of tx_ms and tx_frac and its stores are contiguous, and K = 12 fills the
// lanes the fix's wave-an-epoch geometry leaves idle.  Each thread forms its epoch's frame itself (eight fixed steps and two
// arctangents from the one record its neighbours read too); most of its work is the satellite's two Kepler solutions.
#include "gat_atm_kernels.h"

namespace gat {

namespace {

__global__ __launch_bounds__(kAtmThreads) void atm_kernel(AtmArgs a)
{
    int e, k;
    if (!atm_unit(blockIdx.x, (int)threadIdx.x, a.cells, a.K, &e, &k)) return; // no barrier follows
    atm_cell(a.prm, a.K, e, k, a.eph, a.tx_ms, a.tx_frac, a.rx_ms, a.rx_frac, a.fixes, a.zenith, a.tx_frac_out, a.delay, a.geom, a.ch_status,
             a.ep_status);
}

} // namespace

hipError_t launch_atm(const AtmArgs &a, long long grid, hipStream_t st)
{
    if (grid < 1 || grid > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(atm_kernel, dim3((unsigned)grid), dim3(kAtmThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace gat
