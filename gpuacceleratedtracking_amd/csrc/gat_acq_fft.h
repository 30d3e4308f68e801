// gat_acq_fft.h -- the arithmetic of the FFT acquisition search (include/gat.h gat_acquire_fft), written once for the device kernels
// (gat_acq_fft.hip), for the host twin (gat_acquire_fft_host, gat_acq_fft_api.cpp) and for a stand-alone program
// (tests/acqfftplan): hipcc and plain g++ compile the same text.  With F = 2^L > N, Jseg = F - N + 1 and the plan of
// gat_acq_fft_plan.h, for block b, antenna m (unit u = b M + m), Doppler bin i, PRN p and lag segment g every value is ONE
// sequence of float32 operations (phases in double):
//     step_i  = (if_hz + (f_first + i f_step)) / fs,  th = (double)n * step_i,  (c, s) = fir_sincos(th - rint(th))
//     w[n]    = (fma(xr, c, xi * s), fma(xi, c, -(xr * s)))  for n < N,  +0 for N <= n < F            (the conjugate wipe-off)
//     c_g[n'] = (chip[acq_fft_chip_index(fc / fs, tau_b, n' + first_shift + g Jseg)], +0),  0 <= n' < F,
//               tau_b = fmod(fc / fs * (double)(b * block_stride), Lc): the correlator's chip edges (gat_phase.h chip_index)
//     W, C_g  = T(w), T(c_g);  T = gat_spec.h's radix-2 decimation in time on the bit-reversed input, stages j = 0 .. L - 1,
//               spec_butterfly with spec_twiddle(k F / (2h), F)
//     Y[q]    = C_g[q] * W[(F - q) mod F] = (fma(-C_im, W_im, C_re * W_re), fma(C_im, W_re, C_re * W_im))
//     R[l]    = T(Y)[(F - l) mod F]  for the lags 0 <= l < Jseg (F times the linear correlation sum_n w[n] c_g[n + l])
//     v       = spec_power(R[l]) * 2^(-2 L)                                                           (exact scaling)
//     P[p,i,j] = sum over the unit groups k = 0 .. Gu - 1, in order, of (sum over the units u = k, k + Gu, ... in order of v),
//               each sum in float32, the inner one starting from its first term, at (g, l) = the bin's segment and lag
// With Gu = 1 that is the float32 sum over b (outer) and m (inner).  Gu is a parameter of the plan (the device takes it from its
// compute-unit count), so the twin takes it as an argument.  How many stages run between two trips through LDS or memory, which
// lane holds a value, and how the Doppler bins and the units are batched change no operand and no order.
#pragma once

#include "gat_acq_fft_plan.h"
#include "gat_spec.h"

namespace gat {

// chip index of sample x: gat_phase.h's chip_index operation for operation (an unfused double multiply and add, the floor, the
// float-reciprocal modulo with its two corrections)
GAT_HD inline int acq_fft_chip_index(double ratio, double tau, int x, int Lc, float inv_lc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    const double ph = __dadd_rn(__dmul_rn(ratio, (double)x), tau);
#else
    volatile double t = ratio * (double)x;
    const double ph = t + tau;
#endif
    const int ip = (int)__builtin_floor(ph);
    const float q = __builtin_floorf(spec_mul((float)ip, inv_lc));
    int r = ip - (int)q * Lc;
    r += (r < 0) ? Lc : 0;
    r -= (r >= Lc) ? Lc : 0;
    return r;
}

GAT_HD inline double acq_fft_step(double if_hz, double f_first, double f_step, int i, double fs) { return (if_hz + (f_first + (double)i * f_step)) / fs; }

GAT_HD inline double acq_fft_tau(double ratio, long long b, long long block_stride, int Lc) { return __builtin_fmod(ratio * (double)(b * block_stride), (double)Lc); }

GAT_HD inline void acq_fft_wipe(float xr, float xi, long long n, double step, float &wr, float &wi)
{
    const double th = (double)n * step;
    float c, s;
    fir_sincos(th - __builtin_rint(th), c, s);
    wr = __builtin_fmaf(xr, c, spec_mul(xi, s));
    wi = __builtin_fmaf(xi, c, -spec_mul(xr, s));
}

GAT_HD inline void acq_fft_product(float cr, float ci, float wr, float wi, float &yr, float &yi)
{
    yr = __builtin_fmaf(-ci, wi, spec_mul(cr, wr));
    yi = __builtin_fmaf(ci, wr, spec_mul(cr, wi));
}

GAT_HD inline float acq_fft_scale(int L) { return __builtin_ldexpf(1.0f, -2 * L); }

GAT_HD inline float acq_fft_term(float rr, float ri, float scale) { return spec_mul(spec_power(rr, ri), scale); }

// T in place on the bit-reversed array
inline void acq_fft_host_transform(float *vr, float *vi, int L, const float *twr, const float *twi)
{
    const int F = 1 << L;
    for (int j = 0; j < L; ++j) {
        const int h = 1 << j, shift = L - 1 - j;
        for (int g = 0; g < F; g += 2 * h)
            for (int k = 0; k < h; ++k)
                spec_butterfly(vr[g + k], vi[g + k], vr[g + k + h], vi[g + k + h], twr[(size_t)k << shift], twi[(size_t)k << shift]);
    }
}

// The rule as plain loops over host memory, for a call the plan has accepted with the transform length and the group count
// forced.  codes: [rows][code_row_stride] chips, prns: rows.  Reads samples [0, N) of every (block, antenna) and chips [0, Lc) of
// the rows named; writes the P * D * J sums.
inline void acq_fft_host_run(const gat_signal_desc *sig, const int8_t *codes, int code_row_stride, const int32_t *prns, double fs,
                             const gat_acq_config &cfg, const AcqFftPlan &pl, float *power)
{
    const int L = pl.L, F = 1 << L, M = pl.M, D = pl.D, J = pl.J, Gu = pl.Gu, Lc = cfg.code_length;
    const long long N = pl.N, units = pl.units;
    const double ratio = cfg.code_freq_hz / fs;
    const float inv_lc = 1.0f / (float)Lc, scale = acq_fft_scale(L);
    std::vector<float> twr((size_t)F / 2), twi((size_t)F / 2);
    for (int i = 0; i < F / 2; ++i) spec_twiddle(i, F, twr[(size_t)i], twi[(size_t)i]);
    // W of every (unit, Doppler bin)
    std::vector<float> Wr((size_t)units * D * F), Wi((size_t)units * D * F);
    for (long long u = 0; u < units; ++u) {
        const long long b = u / M, m = u % M;
        const size_t base = (size_t)b * (size_t)sig->block_stride + (size_t)m * (size_t)sig->ant_stride;
        for (int i = 0; i < D; ++i) {
            float *vr = &Wr[((size_t)u * D + i) * F], *vi = &Wi[((size_t)u * D + i) * F];
            const double step = acq_fft_step(cfg.if_hz, cfg.doppler_first_hz, cfg.doppler_step_hz, i, fs);
            for (int n = 0; n < F; ++n) {
                float wr = 0.0f, wi = 0.0f;
                if (n < N) {
                    float xr, xi;
                    host_load_sample(sig, base + (size_t)n, &xr, &xi);
                    acq_fft_wipe(xr, xi, n, step, wr, wi);
                }
                const unsigned q = spec_bitrev((unsigned)n, L);
                vr[q] = wr, vi[q] = wi;
            }
            acq_fft_host_transform(vr, vi, L, twr.data(), twi.data());
        }
    }
    std::vector<float> Cr((size_t)pl.B * pl.G * F), Ci((size_t)pl.B * pl.G * F), yr((size_t)F), yi((size_t)F), slice((size_t)Gu * J);
    for (int p = 0; p < pl.P; ++p) {
        const int8_t *code = codes + (size_t)prns[p] * (size_t)code_row_stride;
        for (int b = 0; b < pl.B; ++b) {
            const double tau = acq_fft_tau(ratio, b, sig->block_stride, Lc);
            for (int g = 0; g < pl.G; ++g) {
                float *vr = &Cr[((size_t)b * pl.G + g) * F], *vi = &Ci[((size_t)b * pl.G + g) * F];
                for (int n = 0; n < F; ++n) {
                    const unsigned q = spec_bitrev((unsigned)n, L);
                    vr[q] = (float)code[acq_fft_chip_index(ratio, tau, (int)(n + cfg.first_shift + (long long)g * pl.Jseg), Lc, inv_lc)];
                    vi[q] = 0.0f;
                }
                acq_fft_host_transform(vr, vi, L, twr.data(), twi.data());
            }
        }
        for (int i = 0; i < D; ++i) {
            for (int k = 0; k < Gu; ++k)
                for (long long u = k; u < units; u += Gu) {
                    const long long b = u / M;
                    const float *wr = &Wr[((size_t)u * D + i) * F], *wi = &Wi[((size_t)u * D + i) * F];
                    for (int g = 0; g < pl.G; ++g) {
                        const float *cr = &Cr[((size_t)b * pl.G + g) * F], *ci = &Ci[((size_t)b * pl.G + g) * F];
                        for (int q = 0; q < F; ++q) {
                            const unsigned r = spec_bitrev((unsigned)q, L);
                            const int qq = (F - q) & (F - 1);
                            acq_fft_product(cr[q], ci[q], wr[qq], wi[qq], yr[r], yi[r]);
                        }
                        acq_fft_host_transform(yr.data(), yi.data(), L, twr.data(), twi.data());
                        for (long long l = 0; l < pl.Jseg; ++l) {
                            const int j = acq_fft_lag_bin(l, g, pl.Jseg, pl.s, J);
                            if (j < 0) continue;
                            const int idx = (int)((F - l) & (F - 1));
                            const float v = acq_fft_term(yr[(size_t)idx], yi[(size_t)idx], scale);
                            float *o = &slice[(size_t)k * J + j];
                            *o = u == k ? v : *o + v;
                        }
                    }
                }
            float *out = power + ((size_t)p * D + i) * J;
            for (int j = 0; j < J; ++j) {
                float v = slice[(size_t)j];
                for (int k = 1; k < Gu; ++k) v += slice[(size_t)k * J + j];
                out[j] = v;
            }
        }
    }
}

} // namespace gat
