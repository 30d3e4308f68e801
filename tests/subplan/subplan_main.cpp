// Stand-alone check of the subspace layer's pure plans (csrc/gat_eig_plan.h) and of the host twins' loops over them (acc_cov_host_run,
// eig_host_one; the rule of csrc/gat_eig.h), over a few thousand random calls.  Every planned covariance must cover each
// (estimate, channel, chunk, entry) exactly once through the workgroups and threads the kernels are launched with -- in either
// work split --, keep its chunk sums inside the planned scratch, and every planned eigensolver each (matrix, round, item) exactly
// once, each sweep every pair once, with its LDS carve-up inside the planned bytes; every documented refusal must return its code
// with nothing planned.  The twins then run on heap buffers of exactly the extents the calls describe -- padded block strides, a
// last partial chunk, a last partial estimate, R = 0, subsets of the outputs --, so that AddressSanitizer sees any read or write
// outside them.  Built with -fsanitize=address,undefined by tests/test_subspace_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_eig.h"
#include "gat_eig_plan.h"

using namespace gat;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            if (++failures <= 20) {                       \
                std::printf("FAIL %s:%d: ", #cond, __LINE__); \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

const void *const kGiven = reinterpret_cast<const void *>(uintptr_t(0x9000));

AccCovCall cov_call(long long stride, int B, int K, int L, int M, int tap, int bpe)
{
    return AccCovCall{kGiven, kGiven, stride, B, K, L, M, tap, bpe, kGiven, kGiven};
}
EigCall eig_call(int n, int Q, int R, unsigned outs = 7, uint32_t flags = 0)
{
    return EigCall{kGiven, kGiven, n, Q, R, flags, outs & 1 ? kGiven : nullptr, outs & 2 ? kGiven : nullptr, outs & 2 ? kGiven : nullptr,
                   outs & 4 ? kGiven : nullptr};
}

template <class P>
P untouched_plan()
{
    P p;
    std::memset(&p, 0x5a, sizeof p);
    return p;
}
template <class P>
bool untouched(const P &p)
{
    const P q = untouched_plan<P>();
    return std::memcmp(&p, &q, sizeof p) == 0;
}
void expect_cov_refusal(const AccCovCall &a, int code, const char *what)
{
    AccCovPlan p = untouched_plan<AccCovPlan>();
    const Refusal r = acc_cov_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}
void expect_eig_refusal(const EigCall &a, int code, const char *what)
{
    EigPlan p = untouched_plan<EigPlan>();
    const Refusal r = eig_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.code == GAT_OK || r.msg != nullptr, "%s: a refusal without a message", what);
    CHECK(untouched(p), "%s: a refused call planned something", what);
}

// walks the launches as the kernels do and counts every (estimate, channel, block, entry)
void check_cov_cover(const AccCovPlan &p, int bpe_arg)
{
    const int bpe = bpe_arg <= 0 || bpe_arg > p.B ? p.B : bpe_arg;
    CHECK(p.bpe == bpe && p.E == (p.B + bpe - 1) / bpe && p.C == (bpe + GAT_ACC_COV_CHUNK - 1) / GAT_ACC_COV_CHUNK && p.T == p.M * (p.M + 1) / 2,
          "counts E %d C %d T %d", p.E, p.C, p.T);
    CHECK(p.split == (p.C >= 2 && (long long)p.E * p.K < kCovFillGroups), "split %d", (int)p.split);
    CHECK(p.lds_bytes == 2 * kCovPiece * p.M * 4 && p.lds_bytes <= 64 * 1024, "lds %d", p.lds_bytes);
    // hit[(k * B + b) * T + t]: how often block b of channel k enters entry t; part[...]: the chunk sums written and read
    std::vector<unsigned char> hit((size_t)p.K * p.B * p.T, 0), entry((size_t)p.M * p.M, 0);
    for (int t = 0; t < p.T; ++t) {
        int i, j;
        cov_entry(t, &i, &j);
        CHECK(i >= 0 && i < p.M && j >= 0 && j <= i && i * (i + 1) / 2 + j == t, "entry %d -> (%d, %d)", t, i, j);
        if (i >= 0 && i < p.M && j >= 0 && j <= i) ++entry[(size_t)i * p.M + j];
    }
    for (int i = 0; i < p.M; ++i)
        for (int j = 0; j <= i; ++j) CHECK(entry[(size_t)i * p.M + j] == 1, "entry (%d, %d) covered %d times", i, j, entry[(size_t)i * p.M + j]);
    auto walk = [&](int k, int first, int count) {
        CHECK(first >= 0 && count >= 1 && count <= GAT_ACC_COV_CHUNK && first + count <= p.B, "chunk %d + %d of %d", first, count, p.B);
        for (int th = 0; th < kCovThreads; ++th)
            for (int v = 0; v < kCovEntriesPerThread; ++v) {
                const int t = v * kCovThreads + th;
                if (t >= p.T) continue;
                for (int b = first; b < first + count && b < p.B; ++b) ++hit[((size_t)k * p.B + b) * p.T + t];
            }
    };
    CHECK(kCovEntriesPerThread * kCovThreads >= p.T, "a thread's entries do not reach T");
    if (p.split) {
        const size_t plane = (size_t)p.E * p.K * p.C * p.T;
        CHECK(p.off_re % 256 == 0 && p.off_im % 256 == 0 && p.off_re + plane * 8 <= p.off_im && p.off_im + plane * 8 <= p.bytes && p.bytes <= kEigMaxScratch,
              "scratch %zu %zu %zu for %zu", p.off_re, p.off_im, p.bytes, plane);
        CHECK(p.g_chunk == (long long)p.E * p.K * p.C, "chunk workgroups %lld", p.g_chunk);
        std::vector<unsigned char> written(plane, 0);
        for (long long u = 0; u < p.g_chunk + 3; ++u) {
            int e, k, c, b0, n, first, count;
            if (!cov_split_unit(u, p.E, p.K, p.C, &e, &k, &c)) {
                CHECK(u >= p.g_chunk, "unit %lld is not decoded", u);
                continue;
            }
            CHECK(u < p.g_chunk && e >= 0 && e < p.E && k >= 0 && k < p.K && c >= 0 && c < p.C, "unit (%d, %d, %d)", e, k, c);
            cov_estimate(e, p.bpe, p.B, &b0, &n);
            if (!cov_chunk(c, b0, n, &first, &count)) continue;
            walk(k, first, count);
            for (int t = 0; t < p.T; ++t) ++written[(size_t)u * p.T + t];
        }
        CHECK(p.g_reduce * kCovThreads >= (long long)p.E * p.K * p.T && (p.g_reduce - 1) * kCovThreads < (long long)p.E * p.K * p.T, "reduce workgroups %lld", p.g_reduce);
        std::vector<unsigned char> out((size_t)p.E * p.K * p.T, 0);
        for (long long v = 0; v < p.g_reduce * kCovThreads; ++v) {
            long long ek;
            int t, b0, n;
            if (!cov_reduce_unit(v, p.E, p.K, p.T, &ek, &t)) continue;
            CHECK(ek >= 0 && ek < (long long)p.E * p.K && t >= 0 && t < p.T, "reduce unit (%lld, %d)", ek, t);
            ++out[(size_t)ek * p.T + t];
            cov_estimate((int)(ek / p.K), p.bpe, p.B, &b0, &n);
            for (int c = 0; c < cov_chunks(n); ++c) {
                const size_t o = ((size_t)ek * p.C + c) * p.T + t;
                CHECK(o < plane && written[o] == 1, "the reduction reads a chunk sum written %d times", o < plane ? written[o] : -1);
                if (o < plane) written[o] = 2;
            }
        }
        for (unsigned char h : out) CHECK(h == 1, "an (estimate, channel, entry) reduced %d times", h);
        for (unsigned char h : written) CHECK(h != 1, "a chunk sum is written and never read");
    } else {
        CHECK(p.bytes == 0 && p.g_reduce == 0 && p.g_chunk == (long long)p.E * p.K, "direct plan: %zu bytes, %lld + %lld workgroups", p.bytes, p.g_chunk, p.g_reduce);
        for (long long u = 0; u < p.g_chunk + 3; ++u) {
            int e, k, b0, n;
            if (!cov_direct_unit(u, p.E, p.K, &e, &k)) {
                CHECK(u >= p.g_chunk, "unit %lld is not decoded", u);
                continue;
            }
            CHECK(u < p.g_chunk && e >= 0 && e < p.E && k >= 0 && k < p.K, "unit (%d, %d)", e, k);
            cov_estimate(e, p.bpe, p.B, &b0, &n);
            for (int c = 0; c < cov_chunks(n); ++c) {
                int first, count;
                CHECK(cov_chunk(c, b0, n, &first, &count), "chunk %d of %d blocks", c, n);
                walk(k, first, count);
            }
        }
    }
    for (unsigned char h : hit) CHECK(h == 1, "a (channel, block, entry) covered %d times", h);
    gat_subspace_plan_info rep{};
    subspace_report(&p, nullptr, &rep);
    CHECK(rep.struct_size == sizeof rep && rep.num_estimates == p.E && rep.chunks_per_estimate == p.C && rep.cov_split == (int)p.split &&
              rep.cov_workgroups == p.g_chunk && rep.cov_reduce_workgroups == p.g_reduce && rep.scratch_bytes == (int64_t)p.bytes && rep.eig_workgroups == 0,
          "report");
}

void check_eig_cover(const EigPlan &p, unsigned outs)
{
    const int Q = p.Q;
    CHECK(p.np == ((Q + 1) & ~1) && p.pairs == p.np / 2 && p.ld >= Q && p.ld % 2 == 1 && p.g == p.n, "geometry np %d pairs %d ld %d", p.np, p.pairs, p.ld);
    CHECK((p.threads == 64 || p.threads == 256) && p.threads >= Q && p.threads >= p.pairs, "threads %d", p.threads);
    CHECK(p.want_vec == ((outs & 2) && p.R > 0) && p.want_val == ((outs & 1) != 0) && p.want_status == ((outs & 4) != 0), "wants");
    // the carve-up, in bytes: planes, per-pair, per-column, F, ints
    const size_t planes = (p.want_vec ? 4 : 2) * p.plane;
    CHECK(p.plane == (size_t)Q * p.ld && p.off_vre == 2 * p.plane && p.off_rot == planes && p.off_col == p.off_rot + 3 * (size_t)p.pairs &&
              p.off_f == p.off_col + 4 * (size_t)Q && p.off_int == p.off_f + 2,
          "carve-up");
    const size_t end = p.off_int * 8 + ((size_t)p.pairs + 2 * (size_t)Q + 4) * 4;
    CHECK((size_t)p.lds_bytes >= end && (size_t)p.lds_bytes < end + 16 && p.lds_bytes % 16 == 0 && p.lds_bytes <= 160 * 1024, "lds %d for %zu", p.lds_bytes, end);
    // a sweep: every round's pairs are disjoint, every pair of indices meets exactly once, every item is taken once
    std::vector<unsigned char> met((size_t)Q * Q, 0);
    for (int r = 0; r < p.np - 1; ++r) {
        std::vector<unsigned char> used((size_t)Q, 0), col_items((size_t)p.pairs * Q, 0), row_items((size_t)p.pairs * Q, 0);
        int live = 0;
        for (int s = 0; s < p.pairs; ++s) {
            int a, b;
            if (!eig_pair(Q, r, s, &a, &b)) continue;
            CHECK(a >= 0 && a < b && b < Q, "pair (%d, %d) of order %d", a, b, Q);
            if (!(a >= 0 && a < b && b < Q)) continue;
            ++used[(size_t)a], ++used[(size_t)b], ++met[(size_t)a * Q + b], ++live;
        }
        CHECK(live == Q / 2, "round %d has %d pairs", r, live);
        for (unsigned char h : used) CHECK(h <= 1, "an index in %d pairs of one round", h);
        for (int th = 0; th < p.threads; ++th)
            for (int t = th; t < p.pairs * Q + p.threads; t += p.threads) {
                int s, line;
                if (!eig_item(t, p.pairs, Q, &s, &line)) continue;
                CHECK(s >= 0 && s < p.pairs && line >= 0 && line < Q, "item (%d, %d)", s, line);
                ++col_items[(size_t)s * Q + line], ++row_items[(size_t)s * Q + line];
            }
        for (unsigned char h : col_items) CHECK(h == 1, "a (pair, row) taken %d times", h);
        for (unsigned char h : row_items) CHECK(h == 1, "a (pair, column) taken %d times", h);
    }
    for (int a = 0; a < Q; ++a)
        for (int b = a + 1; b < Q; ++b) CHECK(met[(size_t)a * Q + b] == 1, "the pair (%d, %d) meets %d times a sweep", a, b, met[(size_t)a * Q + b]);
    // the closed form is the shifting the rule words
    std::vector<int> idx((size_t)p.np);
    for (int i = 0; i < p.np; ++i) idx[(size_t)i] = i;
    for (int r = 0; r < p.np - 1; ++r) {
        for (int i = 0; i < p.np; ++i) CHECK(eig_idx(p.np, r, i) == idx[(size_t)i], "idx[%d] of round %d", i, r);
        std::vector<int> next(idx);
        for (int i = 1; i < p.np; ++i) next[(size_t)i] = idx[(size_t)(i == 1 ? p.np - 1 : i - 1)];
        idx = next;
    }
    gat_subspace_plan_info rep{};
    subspace_report(nullptr, &p, &rep);
    CHECK(rep.eig_workgroups == p.n && rep.eig_threads == p.threads && rep.eig_lds_bytes == p.lds_bytes && rep.num_estimates == 0, "report");
}

template <class T>
struct Out {
    std::vector<T> v;
    bool given;
    Out(size_t n, bool g) : v(g ? n : 0), given(g) {}
    T *ptr() { return given ? (v.empty() ? reinterpret_cast<T *>(uintptr_t(64)) : v.data()) : nullptr; }
};

void run_cov_host(std::mt19937_64 &rng, int B, int K, int L, int M, int pad, int bpe)
{
    const long long n = (long long)K * L * M, stride = n + pad;
    const size_t extent = (size_t)((B - 1) * stride + n);
    std::vector<float> re(extent), im(extent);
    std::uniform_real_distribution<float> u(-50.f, 50.f);
    for (size_t i = 0; i < extent; ++i) re[i] = u(rng), im[i] = u(rng);
    AccCovCall a = cov_call(B == 1 ? -7 : stride, B, K, L, M, (int)(rng() % (unsigned)L), bpe);
    AccCovPlan p{};
    const Refusal r = acc_cov_plan(a, &p);
    CHECK(r.code == GAT_OK, "host case refused: %s", r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    check_cov_cover(p, bpe);
    std::vector<double> cr((size_t)p.E * K * M * M, -1.0), ci((size_t)p.E * K * M * M, -1.0);
    acc_cov_host_run(p, re.data(), im.data(), a.acc_block_stride, cr.data(), ci.data());
    for (int ek = 0; ek < p.E * K; ++ek)
        for (int i = 0; i < M; ++i)
            for (int j = 0; j <= i; ++j) {
                const size_t lo = ((size_t)ek * M + i) * M + j, up = ((size_t)ek * M + j) * M + i;
                CHECK(cr[lo] == cr[up] && ci[lo] == -ci[up] && (i != j || (ci[lo] == 0.0 && !std::signbit(ci[lo]) && cr[lo] >= 0.0)), "not Hermitian at (%d, %d)", i, j);
            }
}

void run_eig_host(std::mt19937_64 &rng, int n, int Q, int R, unsigned outs, bool f32)
{
    std::normal_distribution<double> g(0.0, 1.0);
    const size_t N = (size_t)n * Q * Q;
    std::vector<double> dre(N), dim(N);
    std::vector<float> fre(N), fim(N);
    for (size_t i = 0; i < N; ++i) dre[i] = g(rng), dim[i] = g(rng), fre[i] = (float)dre[i], fim[i] = (float)dim[i];
    EigCall a = eig_call(n, Q, R, outs, f32 ? GAT_EIG_INPUT_F32 : 0u);
    a.a_re = f32 ? (const void *)fre.data() : dre.data(), a.a_im = f32 ? (const void *)fim.data() : dim.data();
    Out<double> ev((size_t)n * Q, outs & 1), vr((size_t)n * R * Q, outs & 2), vi((size_t)n * R * Q, outs & 2);
    Out<int32_t> st((size_t)n, outs & 4);
    a.eigenvalues = ev.ptr(), a.vec_re = vr.ptr(), a.vec_im = vi.ptr(), a.status = st.ptr();
    EigPlan p{};
    const Refusal r = eig_plan(a, &p);
    CHECK(r.code == GAT_OK, "host case refused: %s", r.msg ? r.msg : "");
    if (r.code != GAT_OK) return;
    check_eig_cover(p, outs);
    for (int m = 0; m < n; ++m) eig_host_one(p, a.a_re, a.a_im, m, ev.ptr(), vr.ptr(), vi.ptr(), st.ptr());
    for (int m = 0; m < n; ++m) {
        if (outs & 4) CHECK(st.v[(size_t)m] >= 0 && st.v[(size_t)m] <= 30, "status %d", st.v[(size_t)m]);
        if (outs & 1)
            for (int i = 1; i < Q; ++i) CHECK(ev.v[(size_t)m * Q + i - 1] >= ev.v[(size_t)m * Q + i], "eigenvalues not descending");
        if ((outs & 2) && R > 0)
            for (int v = 0; v < R; ++v) {
                double norm = 0.0;
                for (int i = 0; i < Q; ++i) {
                    const size_t o = ((size_t)m * R + v) * Q + i;
                    norm += vr.v[o] * vr.v[o] + vi.v[o] * vi.v[o];
                }
                CHECK(std::fabs(norm - 1.0) < 1e-12, "an eigenvector of norm^2 %.17g", norm);
            }
    }
}

} // namespace

int main()
{
    std::mt19937_64 rng(20250317);
    auto pick = [&](long long lo, long long hi) { return (long long)(lo + rng() % (unsigned long long)(hi - lo + 1)); };

    // ---- random plans
    int planned = 0;
    for (int it = 0; it < 3000; ++it) {
        if (it % 3 != 2) {
            const int M = (int)(it % 5 == 0 ? pick(1, 64) : pick(1, 6)), L = (int)pick(1, 5);
            const int B = (int)(it % 7 == 0 ? pick(1, 1500) : pick(1, 300));
            const int K = (int)(it % 31 == 0 ? pick(300, 700) : pick(1, 4));
            const int bpe = (int)(it % 4 == 0 ? 0 : it % 4 == 1 ? pick(1, B + 3) : it % 4 == 2 ? pick(250, 520) : -1);
            const int Kc = (long long)K * B * M * M > 4000000 ? 1 : K; // (the cover's table stays small)
            AccCovPlan p = untouched_plan<AccCovPlan>();
            const Refusal r = acc_cov_plan(cov_call((long long)Kc * L * M + pick(0, 9), B, Kc, L, M, (int)pick(0, L - 1), bpe), &p);
            CHECK(r.code == GAT_OK, "a valid call refused: %s", r.msg ? r.msg : "");
            if (r.code != GAT_OK) continue;
            check_cov_cover(p, bpe);
        } else {
            const int Q = (int)(it % 2 ? pick(1, 64) : pick(1, 9)), R = (int)pick(0, Q);
            const unsigned outs = (unsigned)pick(1, 7);
            EigPlan p = untouched_plan<EigPlan>();
            const Refusal r = eig_plan(eig_call((int)pick(1, 1000), Q, R, outs, (uint32_t)(it & 1)), &p);
            CHECK(r.code == GAT_OK, "a valid call refused: %s", r.msg ? r.msg : "");
            if (r.code != GAT_OK) continue;
            check_eig_cover(p, outs);
        }
        ++planned;
    }
    // both work splits are planned, the limits too
    {
        AccCovPlan p{};
        CHECK(acc_cov_plan(cov_call(6, 700, 2, 3, 1, 0, 0), &p).code == GAT_OK && p.split && p.C == 3 && p.g_chunk == 6, "700 blocks of two channels split");
        CHECK(acc_cov_plan(cov_call(600 * 3, 700, 600, 3, 1, 0, 0), &p).code == GAT_OK && !p.split && p.C == 3 && p.g_chunk == 600, "600 channels walk their chunks");
        CHECK(acc_cov_plan(cov_call(6, 700, 2, 3, 1, 0, 256), &p).code == GAT_OK && !p.split && p.E == 3 && p.C == 1, "one chunk an estimate: nothing to split");
        CHECK(acc_cov_plan(cov_call(3, GAT_MAX_MONITOR_BLOCKS, 1, 3, 1, 2, 0), &p).code == GAT_OK && p.bytes <= kEigMaxScratch, "2^20 blocks of one channel");
        CHECK(acc_cov_plan(cov_call(3 * 4096 * 64, 97, GAT_MAX_MONITOR_CHANNELS, 3, GAT_MAX_ARRAY_ANTS, 1, 1), &p).code == GAT_OK && !p.split, "4096 channels of 64 antennas");
        expect_cov_refusal(cov_call(511 * 64, GAT_MAX_MONITOR_BLOCKS, 511, 1, GAT_MAX_ARRAY_ANTS, 0, 0), GAT_ERR_RANGE, "scratch beyond 1 GiB");
        EigPlan e{};
        CHECK(eig_plan(eig_call(1, 64, 64), &e).code == GAT_OK && e.lds_bytes > 128 * 1024 && e.lds_bytes <= 160 * 1024 && e.threads == 256, "order 64 with vectors");
        CHECK(eig_plan(eig_call(1, 64, 64, 5), &e).code == GAT_OK && e.lds_bytes < 72 * 1024 && !e.want_vec, "order 64 without vectors");
        CHECK(eig_plan(eig_call(1, 16, 1), &e).code == GAT_OK && e.threads == 64, "order 16");
    }

    // ---- refusals
    {
        const long long n = 2 * 3 * 2;
        AccCovPlan p{};
        CHECK(acc_cov_plan(cov_call(n, 24, 2, 3, 2, 1, 0), &p).code == GAT_OK, "the base call");
        CHECK(acc_cov_plan(cov_call(n, 24, 2, 3, 2, 1, 0), nullptr).code == GAT_ERR_ARG, "null plan");
        AccCovCall a = cov_call(n, 24, 2, 3, 2, 1, 0);
        a.acc_re = nullptr;
        expect_cov_refusal(a, GAT_ERR_ARG, "null acc_re");
        a = cov_call(n, 24, 2, 3, 2, 1, 0), a.acc_im = nullptr;
        expect_cov_refusal(a, GAT_ERR_ARG, "null acc_im");
        a = cov_call(n, 24, 2, 3, 2, 1, 0), a.cov_re = nullptr;
        expect_cov_refusal(a, GAT_ERR_ARG, "null cov_re");
        a = cov_call(n, 24, 2, 3, 2, 1, 0), a.cov_im = nullptr;
        expect_cov_refusal(a, GAT_ERR_ARG, "null cov_im");
        expect_cov_refusal(cov_call(n, 0, 2, 3, 2, 1, 0), GAT_ERR_ARG, "B = 0");
        expect_cov_refusal(cov_call(n, 24, 0, 3, 2, 1, 0), GAT_ERR_ARG, "K = 0");
        expect_cov_refusal(cov_call(n, 24, 2, 0, 2, 0, 0), GAT_ERR_ARG, "L = 0");
        expect_cov_refusal(cov_call(n, 24, 2, 3, 0, 1, 0), GAT_ERR_ARG, "M = 0");
        expect_cov_refusal(cov_call(2 * 3 * 65, 24, 2, 3, 65, 1, 0), GAT_ERR_RANGE, "M = 65");
        expect_cov_refusal(cov_call(n, GAT_MAX_MONITOR_BLOCKS + 1, 2, 3, 2, 1, 0), GAT_ERR_RANGE, "B above 2^20");
        expect_cov_refusal(cov_call(4097 * 6, 24, 4097, 3, 2, 1, 0), GAT_ERR_RANGE, "K = 4097");
        expect_cov_refusal(cov_call(n, 24, 2, 3, 2, 3, 0), GAT_ERR_RANGE, "tap_index = L");
        expect_cov_refusal(cov_call(n, 24, 2, 3, 2, -1, 0), GAT_ERR_RANGE, "tap_index < 0");
        expect_cov_refusal(cov_call(n - 1, 24, 2, 3, 2, 1, 0), GAT_ERR_ARG, "stride below one block");
        expect_cov_refusal(cov_call(-n, 24, 2, 3, 2, 1, 0), GAT_ERR_ARG, "negative stride");
        CHECK(acc_cov_plan(cov_call(-n, 1, 2, 3, 2, 1, 0), &p).code == GAT_OK, "one block takes any stride");

        EigPlan e{};
        CHECK(eig_plan(eig_call(3, 5, 2), &e).code == GAT_OK, "the base call");
        CHECK(eig_plan(eig_call(3, 5, 2), nullptr).code == GAT_ERR_ARG, "null plan");
        EigCall c = eig_call(3, 5, 2);
        c.a_re = nullptr;
        expect_eig_refusal(c, GAT_ERR_ARG, "null a_re");
        c = eig_call(3, 5, 2), c.a_im = nullptr;
        expect_eig_refusal(c, GAT_ERR_ARG, "null a_im");
        expect_eig_refusal(eig_call(3, 5, 2, 0), GAT_ERR_ARG, "every output null");
        expect_eig_refusal(eig_call(0, 5, 2), GAT_ERR_ARG, "n = 0");
        expect_eig_refusal(eig_call(3, 0, 0), GAT_ERR_RANGE, "Q = 0");
        expect_eig_refusal(eig_call(3, 65, 2), GAT_ERR_RANGE, "Q = 65");
        expect_eig_refusal(eig_call(3, 5, -1), GAT_ERR_RANGE, "R = -1");
        expect_eig_refusal(eig_call(3, 5, 6), GAT_ERR_RANGE, "R = Q + 1");
        c = eig_call(3, 5, 2), c.vec_im = nullptr;
        expect_eig_refusal(c, GAT_ERR_ARG, "vec_re alone");
        c = eig_call(3, 5, 2), c.vec_re = nullptr;
        expect_eig_refusal(c, GAT_ERR_ARG, "vec_im alone");
        expect_eig_refusal(eig_call(3, 5, 2, 7, 2u), GAT_ERR_ARG, "an unknown flag");
    }

    // ---- the host twins on exact extents
    int ran = 0;
    for (int B : {1, 5, 255, 256, 257, 700})
        for (int pad : {0, 5})
            for (int bpe : {0, 1, 256, 300, B, B + 3}) {
                if (bpe == 1 && B > 300) continue;
                run_cov_host(rng, B, (int)pick(1, 3), (int)pick(1, 3), (int)(ran % 5 == 0 ? pick(1, 9) : pick(1, 4)), pad, bpe);
                ++ran;
            }
    run_cov_host(rng, 300, 2, 2, 64, 3, 0), ++ran;
    for (int Q : {1, 2, 3, 4, 5, 8, 16, 17})
        for (int R : {0, 1, Q})
            for (unsigned outs : {7u, 1u, 2u, 4u, 5u, 3u}) {
                run_eig_host(rng, (int)pick(1, 3), Q, R, outs, ran % 2 == 0);
                ++ran;
            }
    run_eig_host(rng, 2, 33, 33, 7, false), ++ran;
    run_eig_host(rng, 1, 64, 1, 7, true), ++ran;
    std::printf("planned %d calls, ran the host twins %d times, %d failures\n", planned, ran, failures);
    return failures ? 1 : 0;
}
