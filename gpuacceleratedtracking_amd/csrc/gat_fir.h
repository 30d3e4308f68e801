// gat_fir.h -- the arithmetic of the sample filter (include/gat.h, "sample filtering"), written once for the device kernels
// (gat_fir.hip), for the host twin (gat_fir_api.cpp) and for a stand-alone program (tests/firplan): hipcc and plain g++ compile
// the same text.  Every output is ONE sequence of float32 operations (the phase: one FP64 FMA) whoever runs it:
//     z     = sum_{t = 0 .. T-1} g[t] * x[p - t],  p = q * D + (T - 1): four FMAs a tap, in tap order, from +0
//     theta = fma((double)P, step, phase),  P = b * block_stride + p: the position in the antenna's stream
//     y     = (c - j s) z,  (c, s) the float polynomial below of exp(j 2 pi theta)
// so the device, the host and any work split agree to the last bit.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_sig_plan.h" // host_load_sample
#include "gat_hd.h"

namespace gat {

// outputs of a block of N samples: the "valid" convolution, decimated (N >= T)
GAT_HD inline long long fir_outputs(long long N, int T, int D) { return (N - T) / D + 1; }

// one tap into the running sum: one FMA per real product, in this order
GAT_HD inline void fir_tap(float &zr, float &zi, float gr, float gi, float xr, float xi)
{
    zr = __builtin_fmaf(gr, xr, zr);
    zr = __builtin_fmaf(-gi, xi, zr);
    zi = __builtin_fmaf(gr, xi, zi);
    zi = __builtin_fmaf(gi, xr, zi);
}

// a float32 product and sum that neither build contracts into an FMA
GAT_HD inline float fir_mul_add(float a, float b, float c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(__fmul_rn(a, b), c);
#else
    volatile float t = a * b;
    return t + c;
#endif
}

// The oscillator: step to [-1/2, 1/2] and phase to [0, 1], as carrier_reduce of gat_phase.h does, so that theta rounds a value
// below P / 2 + 1.  step - rint(step) is exact; phase - floor(phase) is exact except for a negative phase above -2^-53, which
// rounds to 1.0: an error below 2^-54 cycles, inside the bound's phase term.  `rotate` is taken from the caller's values: step == 0 && phase == 0 is the plain filter.
struct FirNco {
    double step, phase;
    int rotate;
};
GAT_HD inline FirNco fir_nco(double step, double phase)
{
    FirNco n;
    n.rotate = !(step == 0.0 && phase == 0.0);
    n.phase = phase - __builtin_floor(phase);
    n.step = step - __builtin_rint(step);
    return n;
}

// exp(j 2 pi theta) for theta in cycles: the octant reduction in double (exact) and the float polynomials of gat_phase.h's
// sincos_cycles, operation for operation
GAT_HD inline void fir_sincos(double theta, float &c, float &s)
{
    const double q = __builtin_rint(theta * 4.0);
    const double r = __builtin_fma(q, -0.25, theta);
    const float a = (float)r * 6.283185307179586f;
    const float a2 = a * a;
    float sp = fir_mul_add(a2, 2.7557319e-6f, -1.9841270e-4f);
    sp = __builtin_fmaf(a2, sp, 8.3333333e-3f);
    sp = __builtin_fmaf(a2, sp, -1.6666667e-1f);
    sp = __builtin_fmaf(a2 * a, sp, a);
    float cp = fir_mul_add(a2, 2.4801587e-5f, -1.3888889e-3f);
    cp = __builtin_fmaf(a2, cp, 4.1666667e-2f);
    cp = __builtin_fmaf(a2, cp, -0.5f);
    cp = __builtin_fmaf(a2, cp, 1.0f);
    const int qi = (int)(long long)q & 3;
    const float cs = (qi & 1) ? sp : cp;
    const float sn = (qi & 1) ? cp : sp;
    c = (qi == 1 || qi == 2) ? -cs : cs;
    s = (qi >= 2) ? -sn : sn;
}

// y = (c - j s) z at stream position P; without rotation y = z bit for bit
GAT_HD inline void fir_rotate(const FirNco &nco, long long P, float zr, float zi, float &yr, float &yi)
{
    if (!nco.rotate) {
        yr = zr, yi = zi;
        return;
    }
    float c, s;
    fir_sincos(__builtin_fma((double)P, nco.step, nco.phase), c, s);
    const float cr = c * zr, ci = c * zi;
    yr = __builtin_fmaf(s, zi, cr);
    yi = __builtin_fmaf(-s, zr, ci);
}

// The rule as a plain loop over host memory, for a call the plan (gat_fir_plan.h) has accepted: the output is float32, planar or
// interleaved.  Reads samples [0, N) of every (block, antenna) and nothing else; writes the Q described outputs of each.
inline void fir_host_run(const gat_signal_desc *sig, int B, const float *taps_re, const float *taps_im, int T, int D, double step, double phase,
                         const gat_signal_desc *out)
{
    const FirNco nco = fir_nco(step, phase);
    const long long Q = fir_outputs(sig->num_samples, T, D);
    float *o_re = static_cast<float *>(const_cast<void *>(out->re)), *o_im = static_cast<float *>(const_cast<void *>(out->im));
    for (int b = 0; b < B; ++b)
        for (int m = 0; m < sig->num_ants; ++m) {
            const size_t base = (size_t)b * (size_t)sig->block_stride + (size_t)m * (size_t)sig->ant_stride;
            const size_t obase = (size_t)b * (size_t)out->block_stride + (size_t)m * (size_t)out->ant_stride;
            for (long long q = 0; q < Q; ++q) {
                const long long p = q * D + (T - 1);
                float zr = 0.0f, zi = 0.0f;
                for (int t = 0; t < T; ++t) {
                    float xr, xi;
                    host_load_sample(sig, base + (size_t)(p - t), &xr, &xi);
                    fir_tap(zr, zi, taps_re[t], taps_im[t], xr, xi);
                }
                float yr, yi;
                fir_rotate(nco, (long long)b * (long long)sig->block_stride + p, zr, zi, yr, yi);
                if (out->layout == GAT_LAYOUT_PLANAR)
                    o_re[obase + (size_t)q] = yr, o_im[obase + (size_t)q] = yi;
                else
                    o_re[2 * (obase + (size_t)q)] = yr, o_re[2 * (obase + (size_t)q) + 1] = yi;
            }
        }
}

} // namespace gat
