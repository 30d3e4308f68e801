// gat_spec.h -- the arithmetic of the sample spectrum (include/gat.h, "sample spectrum"), written once for the device kernels
// (gat_spec.hip), for the host twin (gat_spec_api.cpp) and for a stand-alone program (tests/specplan): hipcc and plain g++ compile
// the same text.  For block b, antenna m and segment s of F samples every H samples, every value is ONE sequence of float32 operations:
//     v[n]   = w[n] * x[s H + n]                               one rounded product per component
//     tw[i]  = (c, -s), (c, s) = fir_sincos((double)i / F)     0 <= i < F/2: the float polynomial of gat_fir.h (i / F is exact)
//     X      = radix-2 decimation in time on the bit-reversed v, stages j = 0 .. log2F - 1, h = 2^j, group g, k < h:
//                  a = v[2hg + k], b = v[2hg + k + h], W = tw[k F / (2h)]
//                  t_re = fma(-W_im, b_im, W_re * b_re), t_im = fma(W_im, b_re, W_re * b_im)     (the inner product rounded)
//                  a' = a + t, b' = a - t
//     p      = fma(X_im, X_im, X_re * X_re)
//     power[b][m][f] = sum_s p                                 one float32 sum in segment order from +0
// Which lane holds which value, and how many stages run between two trips through LDS, changes no operand and no order of any
// value's operations, so the device, the host and any work split agree to the last bit.  The sum over a block's segments is
// sequential by rule: the work unit is a (block, antenna) pair and is never split; parallelism comes from B * M.
#pragma once

#include "gat_fir.h"
#include "gat_spec_plan.h"

#include <vector>

namespace gat {

// segments of a block of N samples (N >= F): the last (N - F) mod H samples are not used
GAT_HD inline long long spec_segments(long long N, int F, int H) { return (N - F) / H + 1; }

// the L low bits of n, reversed
GAT_HD inline unsigned spec_bitrev(unsigned n, int L)
{
    n = (n >> 16) | (n << 16);
    n = ((n & 0xff00ff00u) >> 8) | ((n & 0x00ff00ffu) << 8);
    n = ((n & 0xf0f0f0f0u) >> 4) | ((n & 0x0f0f0f0fu) << 4);
    n = ((n & 0xccccccccu) >> 2) | ((n & 0x33333333u) << 2);
    n = ((n & 0xaaaaaaaau) >> 1) | ((n & 0x55555555u) << 1);
    return n >> (32 - L);
}

// a float32 product that neither build contracts into a following sum (fir_mul_add's way)
GAT_HD inline float spec_mul(float a, float b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    volatile float t = a * b;
    return t;
#endif
}

// twiddle i of F/2: exp(-j 2 pi i / F) as (c, -s)
GAT_HD inline void spec_twiddle(int i, int F, float &wr, float &wi)
{
    float c, s;
    fir_sincos((double)i / (double)F, c, s);
    wr = c, wi = -s;
}

// one butterfly, in place: (a, b) <- (a + W b, a - W b)
GAT_HD inline void spec_butterfly(float &ar, float &ai, float &br, float &bi, float wr, float wi)
{
    const float tr = __builtin_fmaf(-wi, bi, spec_mul(wr, br));
    const float ti = __builtin_fmaf(wi, br, spec_mul(wr, bi));
    br = ar - tr, bi = ai - ti;
    ar = ar + tr, ai = ai + ti;
}

GAT_HD inline float spec_power(float xr, float xi) { return __builtin_fmaf(xi, xi, spec_mul(xr, xr)); }

// The rule as a plain loop over host memory, for a call the plan (gat_spec_plan.h) has accepted.  Reads samples [0, (S - 1) H + F)
// of every (block, antenna) and nothing else; writes the B * M * F sums.
inline void spec_host_run(const gat_signal_desc *sig, int B, const float *window, int F, int H, float *power)
{
    const int L = spec_ilog2(F), M = sig->num_ants;
    const long long S = spec_segments(sig->num_samples, F, H);
    std::vector<float> twr((size_t)F / 2), twi((size_t)F / 2), vr((size_t)F), vi((size_t)F);
    for (int i = 0; i < F / 2; ++i) spec_twiddle(i, F, twr[(size_t)i], twi[(size_t)i]);
    for (int b = 0; b < B; ++b)
        for (int m = 0; m < M; ++m) {
            const size_t base = (size_t)b * (size_t)sig->block_stride + (size_t)m * (size_t)sig->ant_stride;
            float *out = power + ((size_t)b * (size_t)M + (size_t)m) * (size_t)F;
            for (int f = 0; f < F; ++f) out[f] = 0.0f;
            for (long long s = 0; s < S; ++s) {
                for (int n = 0; n < F; ++n) {
                    float xr, xi;
                    host_load_sample(sig, base + (size_t)(s * H + n), &xr, &xi);
                    const unsigned q = spec_bitrev((unsigned)n, L);
                    vr[q] = spec_mul(window[n], xr), vi[q] = spec_mul(window[n], xi);
                }
                for (int j = 0; j < L; ++j) {
                    const int h = 1 << j, shift = L - 1 - j;
                    for (int g = 0; g < F; g += 2 * h)
                        for (int k = 0; k < h; ++k)
                            spec_butterfly(vr[(size_t)(g + k)], vi[(size_t)(g + k)], vr[(size_t)(g + k + h)], vi[(size_t)(g + k + h)],
                                           twr[(size_t)k << shift], twi[(size_t)k << shift]);
                }
                for (int f = 0; f < F; ++f) out[f] = out[f] + spec_power(vr[(size_t)f], vi[(size_t)f]);
            }
        }
}

} // namespace gat
