// gat_eig_plan.h -- the pure part of gat_accumulator_covariance and gat_hermitian_eig (include/gat.h): their refusals, the counts
// (estimates, chunks, lower-triangle entries), the choice between the two work splits of the covariance, the scratch carve-up, the
// launch geometry with the work units' decoding, the eigensolver's carve-up of its workgroup's LDS, and the host twins' loops.  A
// function of the call's arguments alone.  No HIP call and no HIP header: the device entry points, the host twins and a stand-alone
// test program (tests/subplan) compile the same text.
#pragma once

#include <vector>

#include "gat_eig.h"      // gat.h: the accumulators and their limits are the monitor's (GAT_MAX_MONITOR_BLOCKS / _CHANNELS)
#include "gat_sig_plan.h" // Refusal

namespace gat {

// ---- accumulator covariance ------------------------------------------------------------------------------------------------------
constexpr int kCovThreads = 256;
constexpr int kCovPiece = 32;                                                   // blocks staged in LDS at a time
constexpr int kCovMaxEntries = GAT_MAX_ARRAY_ANTS * (GAT_MAX_ARRAY_ANTS + 1) / 2; // 2080
constexpr int kCovEntriesPerThread = (kCovMaxEntries + kCovThreads - 1) / kCovThreads; // 9
constexpr long long kCovFillGroups = 512; // fewer (estimate, channel) pairs than this: the chunks go to workgroups of their own
constexpr size_t kEigMaxScratch = (size_t)1 << 30;
constexpr long long kEigMaxGrid = 0x7fffffffll;

struct AccCovCall {
    const void *acc_re, *acc_im;
    long long acc_block_stride;
    int B, K, L, M, tap, bpe;
    const void *cov_re, *cov_im;
};

// Work units, one workgroup of kCovThreads threads each:
//   split:   u < E K C:  (e, k, c) = (u / (K C), u / C % K, u % C), the sums of chunk c written to scratch[(u T + t)], t < T
//            (nothing where the estimate has no such chunk), then one THREAD per (e, k, t): v < E K T, (e k, t) = (v / T, v % T)
//   direct:  u < E K:    (e, k) = (u / K, u % K), the workgroup walks the estimate's chunks
// Thread j of a workgroup owns the entries t = j, j + kCovThreads, ... < T.  Scratch (split only): [re | im], each E K C T doubles.
struct AccCovPlan {
    int B, K, L, M, tap, bpe; // bpe: the blocks of a full estimate, 1 .. B
    int E, C, T;              // estimates, chunks of a full estimate, lower-triangle entries
    bool split;
    size_t off_re, off_im, bytes;
    long long g_chunk, g_reduce; // workgroups; g_reduce = 0: no second kernel
    int lds_bytes;
};

inline size_t eig_align(size_t v) { return (v + 255) & ~(size_t)255; }

// the blocks of estimate e: first and count
GAT_HD inline void cov_estimate(int e, int bpe, int B, int *b0, int *n)
{
    *b0 = e * bpe;
    *n = B - *b0 < bpe ? B - *b0 : bpe;
}
GAT_HD inline int cov_chunks(int n) { return (n + GAT_ACC_COV_CHUNK - 1) / GAT_ACC_COV_CHUNK; }
// chunk c of an estimate of n blocks from b0: false where the estimate has no such chunk
GAT_HD inline bool cov_chunk(int c, int b0, int n, int *first, int *count)
{
    const int o = c * GAT_ACC_COV_CHUNK;
    if (o >= n) return false;
    *first = b0 + o;
    *count = n - o < GAT_ACC_COV_CHUNK ? n - o : GAT_ACC_COV_CHUNK;
    return true;
}
GAT_HD inline bool cov_split_unit(long long u, int E, int K, int C, int *e, int *k, int *c)
{
    if (u >= (long long)E * K * C) return false;
    *e = (int)(u / ((long long)K * C)), *k = (int)(u / C % K), *c = (int)(u % C);
    return true;
}
GAT_HD inline bool cov_direct_unit(long long u, int E, int K, int *e, int *k)
{
    if (u >= (long long)E * K) return false;
    *e = (int)(u / K), *k = (int)(u % K);
    return true;
}
GAT_HD inline bool cov_reduce_unit(long long v, int E, int K, int T, long long *ek, int *t)
{
    if (v >= (long long)E * K * T) return false;
    *ek = v / T, *t = (int)(v % T);
    return true;
}

// *plan is written only with GAT_OK.
inline Refusal acc_cov_plan(const AccCovCall &a, AccCovPlan *plan)
{
    if (!a.acc_re || !a.acc_im || !a.cov_re || !a.cov_im || !plan) return {GAT_ERR_ARG, "null argument"};
    if (a.B < 1 || a.K < 1 || a.M < 1 || a.L < 1) return {GAT_ERR_ARG, "num_blocks, num_channels, num_ants and num_taps must be positive"};
    if (a.M > GAT_MAX_ARRAY_ANTS) return {GAT_ERR_RANGE, "more than 64 antennas"};
    if (a.B > GAT_MAX_MONITOR_BLOCKS) return {GAT_ERR_RANGE, "more than 2^20 blocks a call"};
    if (a.K > GAT_MAX_MONITOR_CHANNELS) return {GAT_ERR_RANGE, "more than 4096 channels"};
    if (a.tap < 0 || a.tap >= a.L) return {GAT_ERR_RANGE, "tap_index outside the tap list"};
    if (a.B > 1 && (double)a.acc_block_stride < (double)a.K * (double)a.L * (double)a.M)
        return {GAT_ERR_ARG, "acc_block_stride is below one block's accumulators"};
    AccCovPlan p{};
    p.B = a.B, p.K = a.K, p.L = a.L, p.M = a.M, p.tap = a.tap;
    p.bpe = a.bpe <= 0 || a.bpe > a.B ? a.B : a.bpe;
    p.E = (a.B + p.bpe - 1) / p.bpe;
    p.C = cov_chunks(p.bpe);
    p.T = a.M * (a.M + 1) / 2;
    const long long EK = (long long)p.E * p.K;
    p.split = p.C >= 2 && EK < kCovFillGroups;
    if (p.split) {
        const double plane = (double)EK * (double)p.C * (double)p.T * sizeof(double);
        if (2.0 * plane + 512.0 > (double)kEigMaxScratch)
            return {GAT_ERR_RANGE, "the covariance needs more than 1 GiB of scratch (fewer blocks a call)"};
        p.off_re = 0;
        p.off_im = eig_align((size_t)plane);
        p.bytes = p.off_im + eig_align((size_t)plane);
        p.g_chunk = EK * p.C;
        p.g_reduce = (EK * p.T + kCovThreads - 1) / kCovThreads;
    } else {
        p.g_chunk = EK;
        p.g_reduce = 0;
    }
    if (p.g_chunk > kEigMaxGrid) return {GAT_ERR_RANGE, "more than 2^31 - 1 workgroups (fewer channels or estimates a call)"};
    p.lds_bytes = 2 * kCovPiece * p.M * (int)sizeof(float);
    *plan = p;
    return {GAT_OK, nullptr};
}

// One chunk's sum of entry (i, j) on host memory: blocks first .. first + count in order, from +0
inline void cov_host_chunk(const AccCovPlan &p, const float *acc_re, const float *acc_im, long long stride, int k, int first, int count, int i, int j,
                           double *re, double *im)
{
    double sr = 0.0, si = 0.0;
    for (int b = first; b < first + count; ++b) {
        const size_t o = (p.B > 1 ? (size_t)b * (size_t)stride : 0) + ((size_t)k * p.L + p.tap) * p.M;
        cov_add(acc_re[o + i], acc_im[o + i], acc_re[o + j], acc_im[o + j], sr, si);
    }
    *re = sr, *im = si;
}

// The host twin's loops (gat_accumulator_covariance_host) for a planned call: every pointer host memory.
inline void acc_cov_host_run(const AccCovPlan &p, const float *acc_re, const float *acc_im, long long stride, double *cov_re, double *cov_im)
{
    for (int e = 0; e < p.E; ++e)
        for (int k = 0; k < p.K; ++k) {
            int b0, n;
            cov_estimate(e, p.bpe, p.B, &b0, &n);
            double *out_re = cov_re + ((size_t)e * p.K + k) * p.M * p.M, *out_im = cov_im + ((size_t)e * p.K + k) * p.M * p.M;
            for (int t = 0; t < p.T; ++t) {
                int i, j;
                cov_entry(t, &i, &j);
                double tr = 0.0, ti = 0.0;
                for (int c = 0; c < cov_chunks(n); ++c) {
                    int first, count;
                    double sr, si;
                    cov_chunk(c, b0, n, &first, &count);
                    cov_host_chunk(p, acc_re, acc_im, stride, k, first, count, i, j, &sr, &si);
                    tr += sr, ti += si;
                }
                if (i == j) ti = 0.0;
                out_re[i * p.M + j] = tr, out_im[i * p.M + j] = ti;
                if (i != j) out_re[j * p.M + i] = tr, out_im[j * p.M + i] = -ti;
            }
        }
}

// ---- Hermitian eigensolver -------------------------------------------------------------------------------------------------------
constexpr int kEigThreadsSmall = 64, kEigThreadsLarge = 256, kEigSmallOrder = 16;

struct EigCall {
    const void *a_re, *a_im;
    int n, Q, R;
    uint32_t flags;
    const void *eigenvalues, *vec_re, *vec_im, *status;
};

// One workgroup of `threads` threads per matrix.  A round has `pairs` = n'/2 pair slots (eig_pair: the slot with the dummy index is
// empty); its column phase and its row phase have pairs * Q items each, item t = (pair, row or column) = (t / Q, t % Q), thread j
// taking the items j, j + threads, ...  LDS, in doubles from the base: the planes A re | A im | (with vectors) V re | V im, each
// Q * ld with ld = Q | 1 (odd: a column's elements fall into different banks); then per pair slot c | gr | gi; then per column
// diagonal | factor re | factor im | modulus; then F and one spare; then ints: per pair slot p + 256 q or -1, per column rank |
// largest component, then the sweep's flag and three spare.
struct EigPlan {
    int n, Q, R, np, pairs, ld, threads;
    bool f32, want_vec, want_val, want_status;
    size_t plane;                                   // doubles of one plane
    size_t off_vre, off_rot, off_col, off_f, off_int; // in doubles from the base (off_int: where the ints begin)
    int lds_bytes;
    long long g;
};

GAT_HD inline bool eig_item(int t, int pairs, int Q, int *pair, int *line)
{
    if (t >= pairs * Q) return false;
    *pair = t / Q, *line = t % Q;
    return true;
}

inline Refusal eig_plan(const EigCall &a, EigPlan *plan)
{
    if (!a.a_re || !a.a_im || !plan) return {GAT_ERR_ARG, "null argument"};
    if (a.flags & ~(uint32_t)GAT_EIG_INPUT_F32) return {GAT_ERR_ARG, "unknown flag"};
    if (a.n < 1) return {GAT_ERR_ARG, "num_matrices must be positive"};
    if (a.Q < 1 || a.Q > GAT_MAX_ARRAY_ANTS) return {GAT_ERR_RANGE, "order outside 1 .. 64"};
    if (a.R < 0 || a.R > a.Q) return {GAT_ERR_RANGE, "num_vectors outside 0 .. order"};
    if ((a.vec_re == nullptr) != (a.vec_im == nullptr)) return {GAT_ERR_ARG, "one vector plane without the other"};
    if (!a.eigenvalues && !a.vec_re && !a.status) return {GAT_ERR_ARG, "every output is null"};
    EigPlan p{};
    p.n = a.n, p.Q = a.Q, p.R = a.R, p.np = eig_even(a.Q), p.pairs = p.np / 2, p.ld = a.Q | 1;
    p.threads = a.Q <= kEigSmallOrder ? kEigThreadsSmall : kEigThreadsLarge;
    p.f32 = (a.flags & GAT_EIG_INPUT_F32) != 0;
    p.want_vec = a.vec_re != nullptr && a.R > 0;
    p.want_val = a.eigenvalues != nullptr, p.want_status = a.status != nullptr;
    p.plane = (size_t)p.Q * p.ld;
    p.off_vre = 2 * p.plane;
    p.off_rot = (p.want_vec ? 4 : 2) * p.plane;
    p.off_col = p.off_rot + 3 * (size_t)p.pairs;
    p.off_f = p.off_col + 4 * (size_t)p.Q;
    p.off_int = p.off_f + 2;
    p.lds_bytes = (int)((p.off_int * sizeof(double) + ((size_t)p.pairs + 2 * (size_t)p.Q + 4) * sizeof(int32_t) + 15) & ~(size_t)15);
    p.g = a.n;
    *plan = p;
    return {GAT_OK, nullptr};
}

// One matrix of the host twin (gat_hermitian_eig_host): every pointer host memory, the outputs those of matrix `mat`.
inline void eig_host_one(const EigPlan &p, const void *a_re, const void *a_im, int mat, double *eigenvalues, double *vec_re, double *vec_im, int32_t *status)
{
    const int Q = p.Q, ld = p.ld;
    std::vector<double> are(p.plane, 0.0), aim(p.plane, 0.0), vre(p.want_vec ? p.plane : 0, 0.0), vim(p.want_vec ? p.plane : 0, 0.0);
    const size_t base = (size_t)mat * Q * Q;
    auto in = [&](const void *plane, int i, int j) {
        return p.f32 ? (double)static_cast<const float *>(plane)[base + (size_t)i * Q + j] : static_cast<const double *>(plane)[base + (size_t)i * Q + j];
    };
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j <= i; ++j) {
            const double r = in(a_re, i, j), m = i == j ? 0.0 : in(a_im, i, j);
            are[i * ld + j] = r, aim[i * ld + j] = m;
            are[j * ld + i] = r, aim[j * ld + i] = -m;
        }
    double F = 0.0;
    for (int i = 0; i < Q; ++i)
        for (int j = 0; j < Q; ++j) F += are[i * ld + j] * are[i * ld + j] + aim[i * ld + j] * aim[i * ld + j];
    double *ev = eigenvalues ? eigenvalues + (size_t)mat * Q : nullptr;
    double *wr = p.want_vec ? vec_re + (size_t)mat * p.R * Q : nullptr, *wi = p.want_vec ? vec_im + (size_t)mat * p.R * Q : nullptr;
    if (!(F <= kEigFinite)) {
        const double nan = NAN;
        if (ev)
            for (int i = 0; i < Q; ++i) ev[i] = nan;
        if (wr)
            for (int i = 0; i < p.R * Q; ++i) wr[i] = wi[i] = nan;
        if (status) status[mat] = -2;
        return;
    }
    const double limit = kEigThreshold * F;
    if (p.want_vec)
        for (int i = 0; i < Q; ++i) vre[i * ld + i] = 1.0;
    std::vector<double> c(p.pairs), gr(p.pairs), gi(p.pairs), d(Q);
    std::vector<int> pp(p.pairs), qq(p.pairs);
    int sweeps = 0;
    bool converged = false;
    while (sweeps < GAT_EIG_MAX_SWEEPS) {
        bool any = false;
        for (int r = 0; r < p.np - 1; ++r) {
            for (int s = 0; s < p.pairs; ++s) {
                int a = 0, b = 0;
                const bool live = eig_pair(Q, r, s, &a, &b) && eig_rotation(are[a * ld + a], are[b * ld + b], are[a * ld + b], aim[a * ld + b], limit, &c[s], &gr[s], &gi[s]);
                pp[s] = live ? a : -1, qq[s] = b;
                any = any || live;
            }
            for (int t = 0; t < p.pairs * Q; ++t) {
                int s, row;
                eig_item(t, p.pairs, Q, &s, &row);
                if (pp[s] < 0) continue;
                eig_col_item(are.data(), aim.data(), ld, row, pp[s], qq[s], c[s], gr[s], gi[s]);
                if (p.want_vec) eig_col_item(vre.data(), vim.data(), ld, row, pp[s], qq[s], c[s], gr[s], gi[s]);
            }
            for (int t = 0; t < p.pairs * Q; ++t) {
                int s, col;
                eig_item(t, p.pairs, Q, &s, &col);
                if (pp[s] >= 0) eig_row_item(are.data(), aim.data(), ld, col, pp[s], qq[s], c[s], gr[s], gi[s]);
            }
        }
        if (!any) {
            converged = true;
            break;
        }
        ++sweeps;
    }
    if (status) status[mat] = converged ? sweeps : -1;
    for (int i = 0; i < Q; ++i) d[i] = are[i * ld + i];
    for (int i = 0; i < Q; ++i) {
        const int r = eig_rank(d.data(), Q, i);
        if (ev) ev[r] = d[i];
        if (!p.want_vec || r >= p.R) continue;
        int m;
        double mod, fr, fi;
        eig_phase(vre.data(), vim.data(), ld, Q, i, &m, &mod, &fr, &fi);
        for (int row = 0; row < Q; ++row)
            eig_component(vre[row * ld + i], vim[row * ld + i], row == m, mod, fr, fi, &wr[(size_t)r * Q + row], &wi[(size_t)r * Q + row]);
    }
}

// ---- the public report -----------------------------------------------------------------------------------------------------------
inline void subspace_report(const AccCovPlan *c, const EigPlan *e, gat_subspace_plan_info *out)
{
    const uint32_t size = sizeof(gat_subspace_plan_info);
    *out = gat_subspace_plan_info{};
    out->struct_size = size;
    if (c) {
        out->num_estimates = c->E, out->chunks_per_estimate = c->C, out->cov_split = c->split ? 1 : 0;
        out->cov_workgroups = (int32_t)c->g_chunk, out->cov_threads = kCovThreads, out->cov_lds_bytes = c->lds_bytes;
        out->cov_reduce_workgroups = (int32_t)c->g_reduce;
        out->scratch_bytes = (int64_t)c->bytes;
    }
    if (e) out->eig_workgroups = (int32_t)e->g, out->eig_threads = e->threads, out->eig_lds_bytes = e->lds_bytes;
}

} // namespace gat
