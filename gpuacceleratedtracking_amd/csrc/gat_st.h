// gat_st.h -- the arithmetic of space-time adaptive processing (include/gat.h, "space-time adaptive processing"), written once
// for the device kernels (gat_st.hip), for the host twin (gat_st_api.cpp) and for a stand-alone program (tests/stplan): hipcc and
// plain g++ compile the same text.  The snapshot of a block at sample n, T - 1 <= n < N, is z[q] = x[n - t, m] with q = t * M + m
// (tap 0 the newest sample, the antenna index fastest), and every output of the filter is ONE sequence of float32 FMAs whoever
// runs it:
//     y[n'] = sum_{q = 0 .. Q-1} conj(w[q]) z_q[n' + T - 1]:  st_term per element, in q order, from +0, w narrowed to float32 once
// which is gat_beamform_samples' rule (gat_beam.hip) with the snapshot in place of the antenna vector: T = 1 gives its bits.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_fir.h" // GAT_HD, and with it gat_sig_plan.h: host_load_sample

namespace gat {

// outputs of a block of N samples (N >= T): its snapshots
GAT_HD inline long long st_outputs(long long N, int T) { return N - T + 1; }

// work unit u of a filter call (StPlan, gat_st_plan.h): its block and outputs [n0, n1)
GAT_HD inline void st_unit(long long u, long long chunks, long long chunk, long long outputs, long long *b, long long *n0, long long *n1)
{
    *b = u / chunks;
    *n0 = (u - *b * chunks) * chunk;
    *n1 = *n0 + chunk < outputs ? *n0 + chunk : outputs;
}

// one element of the sum, y += conj(w) z: one FMA per real product, in this order
GAT_HD inline void st_term(float wr, float wi, float xr, float xi, float &yr, float &yi)
{
    yr = __builtin_fmaf(wr, xr, yr);
    yr = __builtin_fmaf(wi, xi, yr);
    yi = __builtin_fmaf(wr, xi, yi);
    yi = __builtin_fmaf(-wi, xr, yi);
}

// The rule as a plain loop over host memory, for a call the plan (gat_st_plan.h) has accepted: w is double [J][M * T] planar, the
// output float32, planar or interleaved.  Reads samples [0, N) of every (block, antenna) and nothing else; writes the N - T + 1
// described outputs of every (block, beam).
inline void st_host_run(const gat_signal_desc *sig, int B, const double *w_re, const double *w_im, int T, int J, const gat_signal_desc *out)
{
    const int M = sig->num_ants, Q = M * T;
    const long long No = st_outputs(sig->num_samples, T);
    float *o_re = static_cast<float *>(const_cast<void *>(out->re)), *o_im = static_cast<float *>(const_cast<void *>(out->im));
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < J; ++j) {
            const size_t base = (size_t)b * (size_t)sig->block_stride;
            const size_t obase = (size_t)b * (size_t)out->block_stride + (size_t)j * (size_t)out->ant_stride;
            for (long long n = 0; n < No; ++n) {
                float yr = 0.0f, yi = 0.0f;
                for (int t = 0; t < T; ++t)
                    for (int m = 0; m < M; ++m) {
                        float xr, xi;
                        host_load_sample(sig, base + (size_t)m * (size_t)sig->ant_stride + (size_t)(n + T - 1 - t), &xr, &xi);
                        const size_t q = (size_t)j * (size_t)Q + (size_t)(t * M + m);
                        st_term((float)w_re[q], (float)w_im[q], xr, xi, yr, yi);
                    }
                if (out->layout == GAT_LAYOUT_PLANAR)
                    o_re[obase + (size_t)n] = yr, o_im[obase + (size_t)n] = yi;
                else
                    o_re[2 * (obase + (size_t)n)] = yr, o_re[2 * (obase + (size_t)n) + 1] = yi;
            }
        }
}

} // namespace gat
