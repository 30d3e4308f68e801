// gat_mon.h -- the tracking monitor's rule (include/gat.h, "tracking monitor"): the prompt of a block, the window sums behind
// C/N0 and phase lock, the symbol sums, the bit-synchronisation energies and the choice of the symbol start, written once for the
// device kernels (gat_mon.hip) and for the host twin (gat_mon_api.cpp), as gat_loop.h is for the loop.  Double precision
// throughout; every sum is sequential from +0 in the stated order; compiled without contraction in both builds, so both give the
// same bits.  No transcendental function and no sqrt: the kernels write raw sums, decibels are made by the caller.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

// One tap of one block's accumulators acc_re / acc_im [K][L][M]: sum_m conj(w[k][m]) * acc[k][l][m] in m order, or the plain sum
// over the antennas with both weight pointers null.  The closed loop's prompt, early and late (gat_loop.h) and the monitor's prompt.
GAT_HD inline void tap_sum(const float *acc_re, const float *acc_im, int k, int L, int l, int M, const double *w_re, const double *w_im,
                           double &re, double &im)
{
    re = im = 0.0;
    if (w_re && w_im) {
        for (int m = 0; m < M; ++m) {
            const size_t o = ((size_t)k * L + l) * M + m;
            const double ar = (double)acc_re[o], ai = (double)acc_im[o], wr = w_re[(size_t)k * M + m], wi = w_im[(size_t)k * M + m];
            re += wr * ar + wi * ai;
            im += wr * ai - wi * ar;
        }
        return;
    }
    for (int m = 0; m < M; ++m) {
        const size_t o = ((size_t)k * L + l) * M + m;
        re += (double)acc_re[o];
        im += (double)acc_im[o];
    }
}

// ---- windows ---------------------------------------------------------------------------------------------------------------------
// the sums of one window, blocks added in order
GAT_HD inline void mon_window_begin(gat_monitor_window &w)
{
    w.sum_p2 = w.sum_p4 = w.sum_d = w.sum_i = w.sum_q = 0.0;
    w.blocks = 0;
}
GAT_HD inline void mon_window_add(gat_monitor_window &w, double I, double Q)
{
    const double p = I * I + Q * Q;
    w.sum_p2 += p;
    w.sum_p4 += p * p;
    w.sum_d += I * I - Q * Q;
    w.sum_i += I;
    w.sum_q += Q;
    w.blocks += 1;
}

// ---- symbols ---------------------------------------------------------------------------------------------------------------------
// S = sum_{i < Pd} overlay[i] * P[b0 + i] (re and im apart) and wbp = sum_i |P[b0 + i]|^2, in i order; pr / pi: one channel's series
GAT_HD inline void mon_symbol(const double *pr, const double *pi, long long b0, int Pd, const int8_t *overlay, double &sr, double &si, double &wbp)
{
    sr = si = wbp = 0.0;
    for (int i = 0; i < Pd; ++i) {
        const double I = pr[b0 + i], Q = pi[b0 + i], o = (double)overlay[i];
        sr += o * I;
        si += o * Q;
        wbp += I * I + Q * Q;
    }
}
// |S|^2 of symbol j of the candidate start c: one term of E[c]
GAT_HD inline double mon_symbol_energy(const double *pr, const double *pi, int c, long long j, int Pd, const int8_t *overlay)
{
    double sr, si, wbp;
    mon_symbol(pr, pi, c + j * Pd, Pd, overlay, sr, si, wbp);
    return sr * sr + si * si;
}

// ---- the channel record ----------------------------------------------------------------------------------------------------------
GAT_HD inline int mon_mod(long long v, int Pd)
{
    const long long r = v % Pd;
    return (int)(r < 0 ? r + Pd : r);
}
// e: E[0 .. Pd) of the channel (J > 0), B blocks, J = the search's symbols per candidate; forced: config.symbol_offset
GAT_HD inline void mon_pick(const double *e, int Pd, long long B, long long J, int forced, long long first_block, gat_monitor_channel &ch)
{
    int c = -1;
    if (forced >= 0)
        c = mon_mod((long long)forced - first_block, Pd);
    else if (J > 0) {
        c = 0;
        for (int i = 1; i < Pd; ++i)
            if (e[i] > e[c]) c = i; // the lowest c with the largest E
    }
    ch.start = c;
    ch.symbol_offset = c < 0 ? -1 : mon_mod(first_block + c, Pd);
    ch.num_symbols = c < 0 || B < c ? 0 : (int32_t)((B - c) / Pd);
    ch.reserved = 0;
    ch.e_max = c >= 0 && J > 0 ? e[c] : 0.0;
    double second = 0.0;
    bool any = false;
    if (c >= 0 && J > 0)
        for (int i = 0; i < Pd; ++i)
            if (i != c && (!any || e[i] > second)) second = e[i], any = true;
    ch.e_second = any ? second : 0.0;
}

} // namespace gat
