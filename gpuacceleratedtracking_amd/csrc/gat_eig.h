// gat_eig.h -- the subspace layer's rule (include/gat.h, "subspace"): one term and one chunk of the accumulators' covariance, and the
// cyclic Jacobi eigensolver -- the round-robin pairing, the rotation of a pair, the update of two columns and of two rows, the
// ordering and the phase of the eigenvectors --, written once for the device kernels (gat_eig.hip) and for the host twins
// (gat_eig_plan.h, gat_eig_api.cpp), as gat_mon.h is for the monitor.  Double precision throughout, every expression evaluated
// as written, compiled without contraction in both builds, sqrt and / IEEE as in gat_array.h: both give the same bits.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

constexpr double kEigFinite = 1.79769313486231570815e308;
constexpr double kEigThreshold = 4.930380657631323783823303533017413935e-32; // 2^-104

// ---- accumulator covariance ------------------------------------------------------------------------------------------------------
// lower-triangle entry t = i (i + 1) / 2 + j, j <= i
GAT_HD inline void cov_entry(int t, int *i, int *j)
{
    int r = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while (r * (r + 1) / 2 > t) --r;
    while ((r + 1) * (r + 2) / 2 <= t) ++r;
    *i = r, *j = t - r * (r + 1) / 2;
}
// the term x_i conj(x_j) of one block added to a chunk's sum
GAT_HD inline void cov_add(float xri, float xii, float xrj, float xij, double &re, double &im)
{
    const double ar = (double)xri, ai = (double)xii, br = (double)xrj, bi = (double)xij;
    re += ar * br + ai * bi;
    im += ai * br - ar * bi;
}

// ---- eigensolver: the ordering ---------------------------------------------------------------------------------------------------
constexpr int eig_even(int Q) { return (Q + 1) & ~1; }
// position i of idx in round r of a sweep (r in 0 .. n'-2): position 0 stays, the others move one place on every round
GAT_HD inline int eig_idx(int np, int r, int i)
{
    if (i == 0) return 0;
    int v = (i - 1 - r) % (np - 1);
    if (v < 0) v += np - 1;
    return 1 + v;
}
// pair i < n'/2 of round r; false: the pair holds the dummy index
GAT_HD inline bool eig_pair(int Q, int r, int i, int *p, int *q)
{
    const int np = eig_even(Q), a = eig_idx(np, r, i), b = eig_idx(np, r, np - 1 - i);
    if (a >= Q || b >= Q) return false;
    *p = a < b ? a : b, *q = a < b ? b : a;
    return true;
}

// ---- eigensolver: one pair -------------------------------------------------------------------------------------------------------
// c and g = s u from A[p][p], A[q][q] and b = A[p][q]; false: the pair is not rotated (c and g untouched)
GAT_HD inline bool eig_rotation(double app, double aqq, double br, double bi, double limit, double *c, double *gr, double *gi)
{
    const double b2 = br * br + bi * bi;
    if (!(b2 > limit)) return false;
    const double ab = sqrt(b2);
    const double ur = br / ab, ui = bi / ab;
    const double tau = (aqq - app) / (2.0 * ab);
    const double at = tau < 0.0 ? -tau : tau;
    const double d = at + sqrt(1.0 + tau * tau);
    const double t = tau < 0.0 ? -1.0 / d : 1.0 / d;
    const double cc = 1.0 / sqrt(1.0 + t * t);
    const double s = t * cc;
    *c = cc, *gr = s * ur, *gi = s * ui;
    return true;
}
// A <- A J, V <- V J: the elements p and q of one row
GAT_HD inline void eig_cols(double c, double gr, double gi, double &xpr, double &xpi, double &xqr, double &xqi)
{
    const double pr = c * xpr - (gr * xqr + gi * xqi), pi = c * xpi - (gr * xqi - gi * xqr);
    const double qr = (gr * xpr - gi * xpi) + c * xqr, qi = (gr * xpi + gi * xpr) + c * xqi;
    xpr = pr, xpi = pi, xqr = qr, xqi = qi;
}
// A <- J^H A: the elements p and q of one column
GAT_HD inline void eig_rows(double c, double gr, double gi, double &ypr, double &ypi, double &yqr, double &yqi)
{
    const double pr = c * ypr - (gr * yqr - gi * yqi), pi = c * ypi - (gr * yqi + gi * yqr);
    const double qr = (gr * ypr + gi * ypi) + c * yqr, qi = (gr * ypi - gi * ypr) + c * yqi;
    ypr = pr, ypi = pi, yqr = qr, yqi = qi;
}

// One (pair, row) of the column phase on planes of leading dimension ld
GAT_HD inline void eig_col_item(double *re, double *im, int ld, int row, int p, int q, double c, double gr, double gi)
{
    eig_cols(c, gr, gi, re[row * ld + p], im[row * ld + p], re[row * ld + q], im[row * ld + q]);
}
// One (pair, column) of the row phase, with the exact zeros of the rotated pair
GAT_HD inline void eig_row_item(double *re, double *im, int ld, int col, int p, int q, double c, double gr, double gi)
{
    eig_rows(c, gr, gi, re[p * ld + col], im[p * ld + col], re[q * ld + col], im[q * ld + col]);
    if (col == p) {
        im[p * ld + p] = 0.0;
        re[q * ld + p] = im[q * ld + p] = 0.0;
    } else if (col == q) {
        im[q * ld + q] = 0.0;
        re[p * ld + q] = im[p * ld + q] = 0.0;
    }
}

// ---- eigensolver: the outputs ----------------------------------------------------------------------------------------------------
// where eigenvalue d[i] goes: descending, ties to the lower index
GAT_HD inline int eig_rank(const double *d, int Q, int i)
{
    int r = 0;
    for (int j = 0; j < Q; ++j) r += (d[j] > d[i] || (d[j] == d[i] && j < i)) ? 1 : 0;
    return r;
}
// the component of column `col` of V with the largest re*re + im*im (the lowest index of the largest), its modulus and the unit
// factor conj(v_m) / |v_m|; a zero column keeps the factor 1
GAT_HD inline void eig_phase(const double *v_re, const double *v_im, int ld, int Q, int col, int *m, double *mod, double *fr, double *fi)
{
    int best = 0;
    double big = -1.0;
    for (int i = 0; i < Q; ++i) {
        const double a = v_re[i * ld + col], b = v_im[i * ld + col], n = a * a + b * b;
        if (n > big) big = n, best = i;
    }
    const double a = v_re[best * ld + col], b = v_im[best * ld + col];
    const double ab = sqrt(a * a + b * b);
    *m = best, *mod = ab;
    if (ab > 0.0)
        *fr = a / ab, *fi = -b / ab;
    else
        *fr = 1.0, *fi = 0.0;
}
// component i of the eigenvector: v f, the largest component as (|v_m|, +0)
GAT_HD inline void eig_component(double vr, double vi, bool largest, double mod, double fr, double fi, double *re, double *im)
{
    if (largest && mod > 0.0) {
        *re = mod, *im = 0.0;
        return;
    }
    *re = vr * fr - vi * fi;
    *im = vr * fi + vi * fr;
}

} // namespace gat
