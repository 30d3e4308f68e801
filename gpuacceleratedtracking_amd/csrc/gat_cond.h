// gat_cond.h -- the per-sample arithmetic of the sample conditioner and the AGC's record (include/gat.h, "sample
// conditioning"), written once for the device kernels (gat_cond.hip) and for the host twins (gat_cond_api.cpp), as gat_loop.h
// and gat_array.h are.  Every value is ONE sequence of float32 (the AGC: FP64) operations whoever runs it, and neither build
// contracts a subtraction and a multiplication into an FMA (the device names the two operations; both builds compile with
// -ffp-contract=off): host and device agree to the last bit.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

// kept iff |re| <= T and |im| <= T on the raw sample: a NaN component fails both ways of writing it, so it blanks at any T
GAT_HD inline bool cond_keep(float re, float im, float T) { return fabsf(re) <= T && fabsf(im) <= T; }

// y = (x - dc) * scale: two roundings
GAT_HD inline float cond_value(float x, float dc, float scale)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(__fsub_rn(x, dc), scale);
#else
    volatile float t = x - dc; // (the host build has no contraction either; volatile keeps the intermediate a float32)
    return t * scale;
#endif
}

// an integer output's code: nearest, ties to even; clamped to +-lim (the most negative code is never written); NaN: 0.
// *clipped: the rounded value was outside +-lim, or y was NaN
GAT_HD inline int cond_code(float y, int lim, bool *clipped)
{
    if (!(y == y)) {
        *clipped = true;
        return 0;
    }
    const float r = rintf(y), l = (float)lim;
    *clipped = r > l || r < -l;
    return r > l ? lim : r < -l ? -lim : (int)r;
}

// One estimate's statistics of one antenna into its next record: FP64, narrowed once.
GAT_HD inline gat_cond_params agc_record(const gat_sample_stats_t &s, double target_rms, double blank_factor, int remove_dc)
{
    gat_cond_params p;
    p.scale = 0.0f;
    p.dc_re = p.dc_im = 0.0f;
    p.threshold = INFINITY;
    if (s.kept <= 0) return p;
    const double kept = (double)s.kept;
    const double sigma = sqrt(s.sum_pow / (2.0 * kept));
    if (!(sigma > 0.0) || !(sigma <= 1.7976931348623157e308)) return p;
    p.scale = (float)(target_rms / sigma);
    if (remove_dc) {
        p.dc_re = (float)(s.sum_re / kept);
        p.dc_im = (float)(s.sum_im / kept);
    }
    if (blank_factor > 0.0) p.threshold = (float)(blank_factor * sigma);
    return p;
}

} // namespace gat
