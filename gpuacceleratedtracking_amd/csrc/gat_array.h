// gat_array.h -- the beamformer weights' arithmetic (include/gat.h gat_array_weights / gat_array_weights_host), written once
// for the device kernels (gat_array.hip) and for the host entry point (gat_codes.cpp), as gat_loop.h is for the loop: FP64
// Cholesky R' = L L^H of the diagonally loaded covariance and the two triangular solves behind
//   MVDR            w = R'^-1 a / (a^H R'^-1 a)
//   power inversion w = R'^-1 e0 / (e0^H R'^-1 e0)
//   conventional    w = a / (a^H a).
// Every element is computed by ONE sequence of operations whoever runs it (the device factorises with one thread per row,
// the host with two loops), and both builds compile without contraction: host and device weights agree to the last bit on
// IEEE hardware.  L is kept as two planes [M][M], lower triangle, real diagonal.
#pragma once

#include <math.h>
#include <stddef.h>

#include "gat.h"
#include "gat_hd.h"

namespace gat {

// R' = R + loading * trace(R) / M * I: what is added to the diagonal
GAT_HD inline double array_loading_term(const float *cov_re, int M, double loading)
{
    double tr = 0.0;
    for (int m = 0; m < M; ++m) tr += (double)cov_re[(size_t)m * M + m];
    return loading * tr / (double)M;
}

// Cholesky, column j: the diagonal element from row j's finished columns.  False: R' is not positive definite.
GAT_HD inline bool array_chol_diag(const float *cov_re, double load, double *l_re, double *l_im, int M, int j)
{
    double d = (double)cov_re[(size_t)j * M + j] + load;
    for (int k = 0; k < j; ++k) {
        const double a = l_re[(size_t)j * M + k], b = l_im[(size_t)j * M + k];
        d -= a * a + b * b;
    }
    const bool ok = d > 0.0 && d <= 1.79769313486231570815e308; // (false for NaN)
    l_re[(size_t)j * M + j] = ok ? sqrt(d) : 0.0;
    l_im[(size_t)j * M + j] = 0.0;
    return ok;
}

// Cholesky, column j, row i > j: L[i][j] = (R[i][j] - sum_{k<j} L[i][k] conj(L[j][k])) / L[j][j]
GAT_HD inline void array_chol_offdiag(const float *cov_re, const float *cov_im, double *l_re, double *l_im, int M, int i, int j)
{
    double sr = (double)cov_re[(size_t)i * M + j], si = (double)cov_im[(size_t)i * M + j];
    for (int k = 0; k < j; ++k) {
        const double ar = l_re[(size_t)i * M + k], ai = l_im[(size_t)i * M + k];
        const double br = l_re[(size_t)j * M + k], bi = l_im[(size_t)j * M + k];
        sr -= ar * br + ai * bi;
        si -= ai * br - ar * bi;
    }
    const double d = l_re[(size_t)j * M + j];
    l_re[(size_t)i * M + j] = sr / d;
    l_im[(size_t)i * M + j] = si / d;
}

// z = R'^-1 a by L y = a, L^H z = y (z_re / z_im: M doubles of work space and result), then w = z / (a^H z).  a_re null: a = e0.
// False (w untouched): a^H R'^-1 a is not positive (or not finite).
GAT_HD inline bool array_solve_weights(const double *l_re, const double *l_im, int M, const double *a_re, const double *a_im, double *z_re,
                                       double *z_im, double *w_re, double *w_im)
{
    for (int i = 0; i < M; ++i) { // forward: y overwrites z
        double sr = a_re ? a_re[i] : (i == 0 ? 1.0 : 0.0), si = a_re ? a_im[i] : 0.0;
        for (int k = 0; k < i; ++k) {
            const double lr = l_re[(size_t)i * M + k], li = l_im[(size_t)i * M + k];
            sr -= lr * z_re[k] - li * z_im[k];
            si -= lr * z_im[k] + li * z_re[k];
        }
        const double d = l_re[(size_t)i * M + i];
        z_re[i] = sr / d;
        z_im[i] = si / d;
    }
    for (int i = M - 1; i >= 0; --i) { // backward with L^H: (L^H)[i][k] = conj(L[k][i])
        double sr = z_re[i], si = z_im[i];
        for (int k = i + 1; k < M; ++k) {
            const double lr = l_re[(size_t)k * M + i], li = -l_im[(size_t)k * M + i];
            sr -= lr * z_re[k] - li * z_im[k];
            si -= lr * z_im[k] + li * z_re[k];
        }
        const double d = l_re[(size_t)i * M + i];
        z_re[i] = sr / d;
        z_im[i] = si / d;
    }
    // c = a^H z = a^H R'^-1 a: real and positive in exact arithmetic; its computed imaginary part is rounding error of the
    // order of eps * cond(R').  Dividing by the complex c keeps the constraint w^H a = 1 to a few eps whatever cond(R') is.
    double cr = 0.0, ci = 0.0;
    if (a_re)
        for (int m = 0; m < M; ++m) {
            cr += a_re[m] * z_re[m] + a_im[m] * z_im[m];
            ci += a_re[m] * z_im[m] - a_im[m] * z_re[m];
        }
    else
        cr = z_re[0], ci = z_im[0];
    const double n = cr * cr + ci * ci;
    if (!(cr > 0.0 && n > 0.0 && n <= 1.79769313486231570815e308)) return false;
    for (int m = 0; m < M; ++m) {
        w_re[m] = (z_re[m] * cr + z_im[m] * ci) / n;
        w_im[m] = (z_im[m] * cr - z_re[m] * ci) / n;
    }
    if (!a_re) w_re[0] = 1.0, w_im[0] = 0.0; // e0^H w = 1 exactly
    return true;
}

// w = a / (a^H a).  False (w untouched): a is zero or not finite.
GAT_HD inline bool array_conventional_weights(int M, const double *a_re, const double *a_im, double *w_re, double *w_im)
{
    double den = 0.0;
    for (int m = 0; m < M; ++m) den += a_re[m] * a_re[m] + a_im[m] * a_im[m];
    if (!(den > 0.0 && den <= 1.79769313486231570815e308)) return false;
    for (int m = 0; m < M; ++m) {
        w_re[m] = a_re[m] / den;
        w_im[m] = a_im[m] / den;
    }
    return true;
}

} // namespace gat
