// Stand-alone check of the work split of the operators that reduce blocks to estimates (csrc/gat_est_plan.h) and of their three
// pure plans: gat_spatial_covariance's (csrc/gat_array_plan.h), gat_sample_stats' (csrc/gat_cond_plan.h) and
// gat_spacetime_covariance's (csrc/gat_st_plan.h).  The split and the batches are swept with free parameters; each plan is swept
// with a few thousand random valid calls, whose launches are walked as the kernels walk them: every (block, sample or snapshot)
// must be covered exactly once, the batches must tile the estimates, the kernel must be chosen exactly under its rule; every
// documented refusal must return its code and a message with nothing planned; and the regimes that tests/test_array_domain_gpu.py
// states for the covariance must come out as literal numbers for every device size.  Built with -fsanitize=address,undefined by
// tests/test_estimate_plan_host.py.  No memory behind the descriptors is ever touched: the plans read addresses, not data.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_array_plan.h"
#include "gat_cond_plan.h"
#include "gat_st_plan.h"

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

constexpr int kCus[] = {64, 80, 104, 128, 228, 256, 304, 512}; // the device sizes every regime must hold for
float *const kCov = reinterpret_cast<float *>(uintptr_t(0xA000));
gat_sample_stats_t *const kStats = reinterpret_cast<gat_sample_stats_t *>(uintptr_t(0xB000));

gat_signal_desc desc(uintptr_t re, uintptr_t im, int layout, int M, long long N, long long as, long long bs)
{
    gat_signal_desc d{};
    d.re = reinterpret_cast<const void *>(re);
    d.im = layout == GAT_LAYOUT_PLANAR ? reinterpret_cast<const void *>(im) : nullptr;
    d.layout = layout;
    d.num_ants = M;
    d.num_samples = N;
    d.ant_stride = as;
    d.block_stride = bs;
    d.chan_stride = 0;
    return d;
}

// The estimating operators' split with free parameters: the batches must tile the estimates, and inside a
// batch the kernels' walk -- estimate e owns blocks [e * bpe, min(B, (e + 1) * bpe)) of its launch and G workgroups; its unit u
// is (block u / splits, segment u % splits); workgroup g takes units g, g + G, ... -- must cover every (block, sample) once.
void sweep_estimate_splits(std::mt19937_64 &rng)
{
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    long batches = 0, batched_calls = 0, split_calls = 0;
    for (int it = 0; it < 3000; ++it) {
        const int B = (int)(it % 3 == 0 ? pick(1, 400) : pick(1, 12));
        const int bpe = (int)(it % 4 == 0 ? B + pick(1, 5) : it % 4 == 1 ? 1 : pick(1, B)); // beyond B; one block; a last estimate that may be short
        const long long round_to = pick(0, 2) == 0 ? pick(1, 9) : 64 * pick(1, 32);
        const long long N = it % 5 == 0 ? pick(1, round_to) : pick(1, 3000); // N < round_to among them
        const long long min_seg = round_to * pick(1, 8);
        const long long want = pick(0, 3) == 0 ? pick(1, 16) : 64 * pick(1, 64);
        const size_t slice = (size_t)pick(1, 40000);
        const int E = (B + bpe - 1) / bpe;
        // a cap that holds every estimate, some of them (E above e_max), or not even one slice
        const size_t cap = it % 3 == 0 ? slice * (size_t)pick(1, E) + (size_t)pick(0, (long long)slice - 1) : it % 3 == 1 ? slice * (size_t)E * 4 : (size_t)pick(1, (long long)slice);
        std::vector<unsigned char> hits((size_t)B * (size_t)N, 0);
        int next_e = 0;
        long here = 0;
        bool split = false;
        for (EstimateBatches t(B, bpe, slice, cap); t.next(); ++here) {
            CHECK(t.e0 == next_e && t.en >= 1 && t.e0 + t.en <= E, "batch [%d, +%d) after %d of %d estimates", t.e0, t.en, next_e, E);
            CHECK((size_t)t.en * slice <= cap || t.en == 1, "a batch of %d estimates beyond the cap", t.en);
            CHECK(t.b0 == t.e0 * bpe && t.bn >= 1 && t.b0 + t.bn <= B && (t.e0 + t.en == E ? t.b0 + t.bn == B : t.bn == t.en * bpe), "batch blocks [%d, +%d)", t.b0, t.bn);
            if (!(t.e0 == next_e && t.en >= 1 && t.b0 >= 0 && t.bn >= 1 && t.b0 + t.bn <= B)) break;
            next_e = t.e0 + t.en;
            const long long per_est = want / t.en < 1 ? 1 : want / t.en;
            const EstimateSplit sp = split_estimate(bpe < t.bn ? bpe : t.bn, N, round_to, min_seg, per_est);
            CHECK(sp.seg_len > 0 && sp.seg_len % round_to == 0, "seg_len %lld for round_to %lld", sp.seg_len, round_to);
            CHECK(sp.splits >= 1 && (sp.splits - 1) * sp.seg_len < N && sp.splits * sp.seg_len >= N, "splits %lld of %lld samples for N %lld", sp.splits, sp.seg_len, N);
            CHECK(sp.splits == 1 || sp.splits <= N / min_seg, "segments below min_seg: %lld splits of N %lld, min_seg %lld", sp.splits, N, min_seg);
            const long long blocks = bpe < t.bn ? bpe : t.bn; // of every estimate but a short last one, whose spare workgroups find no unit
            CHECK(sp.G >= 1 && sp.G <= per_est && sp.G <= blocks * sp.splits, "G %lld for per_est %lld, %lld blocks", sp.G, per_est, blocks);
            if (!(sp.seg_len > 0 && sp.splits >= 1 && sp.G >= 1)) break;
            split |= sp.splits > 1;
            for (int e = 0; e < t.en; ++e) { // the launch sees blocks [0, bn) from the batch's offset
                const int b0 = e * bpe, nb = t.bn - b0 < bpe ? t.bn - b0 : bpe;
                CHECK(nb >= 1, "an estimate without blocks");
                const long long units = (long long)nb * sp.splits;
                for (long long g = 0; g < sp.G; ++g)
                    for (long long u = g; u < units; u += sp.G) {
                        const int b = t.b0 + b0 + (int)(u / sp.splits);
                        const long long n0 = (u % sp.splits) * sp.seg_len, n1 = n0 + sp.seg_len < N ? n0 + sp.seg_len : N;
                        CHECK(b < B && n0 < n1, "unit %lld: block %d samples [%lld, %lld)", u, b, n0, n1);
                        if (!(b < B && n0 < n1)) continue;
                        for (long long n = n0; n < n1; ++n) ++hits[(size_t)b * (size_t)N + (size_t)n];
                    }
            }
        }
        CHECK(next_e == E, "the batches end at estimate %d of %d", next_e, E);
        for (size_t i = 0; i < hits.size(); ++i)
            if (hits[i] != 1) {
                CHECK(false, "estimates: block %zu sample %zu covered %d times", i / (size_t)N, i % (size_t)N, (int)hits[i]);
                break;
            }
        batches += here, batched_calls += here > 1, split_calls += split;
    }
    std::printf("split 3000 estimating calls (%ld in several batches, %ld with split blocks)\n", batched_calls, split_calls);
    CHECK(batches >= 3000 && batched_calls > 300 && split_calls > 300, "the estimate sweep lost its balance");
}

// ---- the three real plans --------------------------------------------------------------------------------------------------------
struct Tally {
    long calls = 0, batched = 0, split = 0, vec = 0;
};

// Walks a plan's launches as the kernels do and counts every (block, sample or snapshot).  tiles: the grid's antenna tiles;
// vec_samples: on a vec plan the layout's samples per 16-byte load, else 0; real_cap: the cap is the plan's own, which holds the
// slices of every workgroup a launch wants (a cap cut for the test holds one slice an estimate, as the batches promise).
// Returns the launches; *any_split: a block was cut.
long walk(const EstimatePlan &p, int tiles, long long vec_samples, bool real_cap, bool *any_split, const char *what)
{
    const int B = p.B, bpe = p.bpe, E = (int)(((long long)B + bpe - 1) / bpe);
    const long long N = p.N;
    std::vector<unsigned char> hits((size_t)B * (size_t)N, 0);
    int next_e = 0;
    long launches = 0;
    CHECK(N >= 1 && p.round_to >= 1 && p.min_seg >= p.round_to && p.workgroups_wanted >= 1 && p.slice_bytes >= 1, "%s: the rule", what);
    for (EstimateLaunches t(p); t.next(); ++launches) {
        CHECK(t.e0 == next_e && t.en >= 1 && t.e0 + t.en <= E, "%s: launch [%d, +%d) after %d of %d estimates", what, t.e0, t.en, next_e, E);
        CHECK(t.b0 == t.e0 * bpe && t.bn >= 1 && t.b0 + t.bn <= B && (t.e0 + t.en == E ? t.b0 + t.bn == B : t.bn == t.en * bpe), "%s: launch blocks [%d, +%d)", what, t.b0, t.bn);
        if (!(t.e0 == next_e && t.en >= 1 && t.b0 >= 0 && t.bn >= 1 && t.b0 + t.bn <= B)) break;
        next_e = t.e0 + t.en;
        CHECK(t.seg_len > 0 && t.seg_len % p.round_to == 0, "%s: seg_len %lld for round_to %lld", what, t.seg_len, p.round_to);
        CHECK(vec_samples == 0 || t.seg_len % vec_samples == 0, "%s: seg_len %lld cuts a 16-byte load of %lld samples", what, t.seg_len, vec_samples);
        CHECK(t.splits >= 1 && (t.splits - 1) * t.seg_len < N && t.splits * t.seg_len >= N, "%s: splits %lld of %lld for N %lld", what, t.splits, t.seg_len, N);
        CHECK(t.splits == 1 || t.splits <= N / p.min_seg, "%s: segments below min_seg", what);
        CHECK(t.G >= 1 && (long long)t.en * t.G * tiles <= 0x7fffffffll, "%s: a grid of %d x %lld x %d workgroups", what, t.en, t.G, tiles);
        CHECK(t.scratch_bytes == (size_t)t.en * (size_t)t.G * p.slice_bytes, "%s: scratch bytes", what);
        CHECK((real_cap ? t.scratch_bytes : (size_t)t.en * p.slice_bytes) <= p.cap_bytes || t.en == 1, "%s: %zu bytes of scratch for %d estimates", what, t.scratch_bytes, t.en);
        if (!(t.seg_len > 0 && t.splits >= 1 && t.G >= 1)) break;
        *any_split |= t.splits > 1;
        for (int e = 0; e < t.en; ++e) { // the launch sees blocks [0, bn) from its offset
            const int b0 = e * bpe, nb = t.bn - b0 < bpe ? t.bn - b0 : bpe;
            CHECK(nb >= 1, "%s: an estimate without blocks", what);
            const long long units = (long long)nb * t.splits;
            for (long long g = 0; g < t.G; ++g)
                for (long long u = g; u < units; u += t.G) {
                    const int b = t.b0 + b0 + (int)(u / t.splits);
                    const long long n0 = (u % t.splits) * t.seg_len, n1 = n0 + t.seg_len < N ? n0 + t.seg_len : N;
                    CHECK(b < B && n0 < n1, "%s: unit %lld: block %d [%lld, %lld)", what, u, b, n0, n1); // no empty segment
                    if (!(b < B && n0 < n1)) continue;
                    for (long long n = n0; n < n1; ++n) ++hits[(size_t)b * (size_t)N + (size_t)n];
                }
        }
    }
    CHECK(next_e == E, "%s: the launches end at estimate %d of %d", what, next_e, E);
    for (size_t i = 0; i < hits.size(); ++i)
        if (hits[i] != 1) {
            CHECK(false, "%s: block %zu element %zu covered %d times", what, i / (size_t)N, i % (size_t)N, (int)hits[i]);
            break;
        }
    return launches;
}

// A call of the sweeps: the host simulator's distribution of shapes (N and B log-uniform, its two skews), bounded in B x N
struct Call {
    gat_signal_desc sig;
    int B, bpe, T, cus;
    bool tidy;
};
Call random_call(std::mt19937_64 &rng, int it, bool taps)
{
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    auto log_uniform = [&](double hi) { return (long long)std::llround(std::exp(std::log(hi) * (double)(rng() >> 11) / 9007199254740992.0)); };
    Call c{};
    const int layout = (int)pick(0, 3);
    c.T = taps ? (int)pick(1, GAT_MAX_ST_TAPS) : 1;
    const int most = GAT_MAX_ARRAY_ANTS / c.T;
    const int M = (int)(it % 2 == 0 ? pick(1, most < 8 ? most : 8) : pick(1, most));
    long long N = log_uniform(300000.0);
    int B = (int)log_uniform(6000.0);
    if (it % 10 == 3) B = (int)pick(4100, 6000), N = pick(1, 40);   // many short blocks: more than any device wants workgroups
    if (it % 10 == 7) B = (int)pick(1, 3), N = pick(20000, 300000); // few long blocks: split
    while ((double)B * (double)N > 5e5) { // bounded: the walk's table
        if (B > 1 && pick(0, 1)) B = (B + 1) / 2;
        else N = (N + 1) / 2;
    }
    if (N < c.T) N = c.T;
    c.B = B;
    c.bpe = (int)(it % 4 == 0 ? 1 : it % 4 == 1 ? B : it % 4 == 2 ? B + pick(1, 5) : pick(1, B));
    c.cus = kCus[pick(0, 7)];
    c.tidy = it % 3 != 0; // aligned base and strides of whole 16-byte loads: the vec kernels' candidates
    const long long v = layout_vec_samples(layout);
    const long long bs = c.tidy ? (N + v - 1) / v * v : N + pick(0, 9);
    const long long as = bs * B + (c.tidy ? v * pick(0, 3) : pick(0, 5));
    const uintptr_t off = c.tidy ? 0 : (uintptr_t)pick(0, 3) * layout_sample_bytes(layout);
    c.sig = desc(0x100000000ull + off, 0x4000000000ull + off, layout, M, N, as, bs);
    return c;
}

// a quarter of the calls are walked a second time with the cap cut to a few slices: below 8193 estimates no real cap makes batches
// (256 MB hold 8192 slices of 64 x 64 antennas), and the walk's rules are the same for any cap
void walk_cut_cap(std::mt19937_64 &rng, int it, EstimatePlan p, int tiles, long long vec_samples, Tally *tally, const char *what)
{
    bool split = false;
    const long launches = walk(p, tiles, vec_samples, true, &split, what);
    CHECK(launches == 1, "%s: %ld launches of %d blocks", what, launches, p.B);
    tally->split += split;
    if (it % 4 != 0) return; // bpe = 1: as many estimates as blocks
    const int E = (p.B + p.bpe - 1) / p.bpe;
    p.cap_bytes = p.slice_bytes * (size_t)(rng() % (uint64_t)E + 1) + (size_t)(rng() % p.slice_bytes);
    tally->batched += walk(p, tiles, vec_samples, false, &split, what) > 1;
}

template <class Plan>
void poison(Plan *p) { std::memset(static_cast<void *>(p), 0x5a, sizeof *p); }
// a refusal derived from a valid call: its code, a message (`msg`: that message), the plan left as it was
template <class Plan, class F>
void expect_refusal(F &&call, int code, const char *what, const char *msg = nullptr)
{
    Plan p, q;
    poison(&p), poison(&q);
    const Refusal r = call(&p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.msg != nullptr && (!msg || std::strcmp(r.msg, msg) == 0), "%s: the message is %s", what, r.msg ? r.msg : "missing");
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: a refused call planned something", what);
}
// what check_desc refuses, each from the valid descriptor s; chan_msg: the plan's own answer to a chan_stride
template <class Plan, class F>
void expect_desc_refusals(const gat_signal_desc &s, int B, F &&call, const char *chan_msg)
{
    gat_signal_desc t = s;
    t.layout = 4;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "bad layout");
    t = s, t.layout = -1;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "negative layout");
    t = s, t.im = s.layout == GAT_LAYOUT_PLANAR ? nullptr : t.re;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "signal planes");
    t = s, t.re = nullptr;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "no signal plane");
    t = s, t.num_samples = 0;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "no samples");
    t = s, t.num_ants = 0;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "no antennas");
    t = s, t.ant_stride = -1;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "negative ant_stride");
    t = s, t.block_stride = -1;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "negative block_stride");
    t = s, t.num_ants = GAT_MAX_ARRAY_ANTS + 1;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_RANGE, "too many antennas", "more than 64 antennas");
    t = s, t.chan_stride = 8;
    expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_UNSUPPORTED, "chan_stride", chan_msg);
    if (s.num_ants > 1) {
        t = s, t.ant_stride = 0;
        expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "zero ant_stride");
        t = s, t.ant_stride = 1ll << 60;
        expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_RANGE, "extent");
    }
    if (B > 1) {
        t = s, t.block_stride = 0;
        expect_refusal<Plan>([&](Plan *p) { return call(&t, p); }, GAT_ERR_ARG, "zero block_stride");
    }
}

constexpr int kSweep = 2000;
const char *const kNull = "null argument";

void sweep_cov_plans(std::mt19937_64 &rng)
{
    const char *const chan = "chan_stride must be 0 (one signal, one covariance)", *const sizes = "num_blocks and blocks_per_estimate must be positive";
    Tally n;
    for (int it = 0; it < kSweep; ++it) {
        const Call c = random_call(rng, it, false);
        const gat_signal_desc &s = c.sig;
        const int M = s.num_ants, B = c.B, bpe = c.bpe;
        const long long v = layout_vec_samples(s.layout);
        CovPlan p;
        poison(&p);
        const Refusal r = cov_plan(&s, B, bpe, kCov, kCov, c.cus, &p);
        CHECK(r.code == GAT_OK, "covariance: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++n.calls;
        const bool rule = M <= kCovSmallMaxAnts && blocks_aligned(&s, B);
        CHECK(p.vec == rule, "covariance: vec %d, the rule says %d", (int)p.vec, (int)rule);
        CHECK(!c.tidy || M > 8 || p.vec, "covariance: an aligned call of %d antennas did not stream", M);
        n.vec += p.vec;
        const EstimatePlan &e = p.est;
        const long long round_to = p.vec ? v * kCovSmallThreads : cov_tile_geom(M).chunk;
        CHECK(e.B == B && e.bpe == bpe && e.N == s.num_samples && e.round_to == round_to && e.min_seg == (p.vec ? 4 : 8) * round_to &&
                  e.workgroups_wanted == (long long)c.cus * (p.vec ? 8 : 4) && e.slice_bytes == (size_t)8 * M * M && e.cap_bytes == kCovScratchCap,
              "covariance: the rule of M %d vec %d", M, (int)p.vec);
        walk_cut_cap(rng, it, e, 1, p.vec ? v : 0, &n, "covariance");

        // the refusals, each from this valid call, in the entry point's order
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(nullptr, 0, bpe, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "null signal", kNull);
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(&s, B, 0, nullptr, kCov, c.cus, q); }, GAT_ERR_ARG, "null cov_re", kNull);
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(&s, B, bpe, kCov, nullptr, c.cus, q); }, GAT_ERR_ARG, "null cov_im", kNull);
        gat_signal_desc t = s;
        t.num_ants = GAT_MAX_ARRAY_ANTS + 1;
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(&t, 0, bpe, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "no blocks", sizes);
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(&s, B, 0, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "no blocks per estimate", sizes);
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(&s, -1, -1, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "negative sizes", sizes);
        t.layout = 4, t.ant_stride = 0; // the antenna limit answers ahead of the shared check's layout and strides
        expect_refusal<CovPlan>([&](CovPlan *q) { return cov_plan(&t, B, bpe, kCov, kCov, c.cus, q); }, GAT_ERR_RANGE, "65 antennas of a bad layout", "more than 64 antennas");
        expect_desc_refusals<CovPlan>(s, B, [&](const gat_signal_desc *d, CovPlan *q) { return cov_plan(d, B, bpe, kCov, kCov, c.cus, q); }, chan);
    }
    std::printf("planned %ld covariance calls (%ld streaming, %ld with split blocks, %ld in several batches)\n", n.calls, n.vec, n.split, n.batched);
    CHECK(n.calls == kSweep && n.vec > kSweep / 5 && n.vec < kSweep * 3 / 5 && n.split > kSweep / 10 && n.batched > kSweep / 10, "the covariance sweep lost its balance");
}

void sweep_stats_plans(std::mt19937_64 &rng)
{
    Tally n;
    for (int it = 0; it < kSweep; ++it) {
        const Call c = random_call(rng, it, false);
        const gat_signal_desc &s = c.sig;
        const int M = s.num_ants, B = c.B, bpe = c.bpe;
        const long long v = layout_vec_samples(s.layout);
        const uint32_t flags = (uint32_t)(rng() & 1u);
        StatsPlan p;
        poison(&p);
        const Refusal r = stats_plan(&s, B, bpe, flags, kStats, c.cus, &p);
        CHECK(r.code == GAT_OK, "statistics: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++n.calls;
        const bool rule = M <= kStatsTile && blocks_aligned(&s, B);
        CHECK(p.vec == rule, "statistics: vec %d, the rule says %d", (int)p.vec, (int)rule);
        CHECK(!c.tidy || M > 8 || p.vec, "statistics: an aligned call of %d antennas did not take 16-byte loads", M);
        n.vec += p.vec;
        // the grid's antenna tiles as the launcher deals them: whole tiles of kStatsTile, then the rest
        CHECK(p.tiles == M / kStatsTile + (M % kStatsTile ? 1 : 0) && p.ant_tile == (M < kStatsTile ? M : kStatsTile) && (!p.vec || p.tiles == 1), "statistics: %d tiles of %d for %d antennas", p.tiles, p.ant_tile, M);
        const EstimatePlan &e = p.est;
        const long long round_to = (long long)kStatsThreads * (p.vec ? v : 1);
        CHECK(e.B == B && e.bpe == bpe && e.N == s.num_samples && e.round_to == round_to && e.min_seg == 4 * round_to && e.workgroups_wanted == (long long)c.cus * 8 &&
                  e.slice_bytes == M * sizeof(gat_sample_stats_t) && e.cap_bytes == kStatsScratchCap,
              "statistics: the rule of M %d vec %d", M, (int)p.vec);
        walk_cut_cap(rng, it, e, p.tiles, p.vec ? v : 0, &n, "statistics");

        // the refusals, each from this valid call, in the entry point's order
        expect_refusal<StatsPlan>([&](StatsPlan *q) { return stats_plan(&s, B, 0, flags, nullptr, c.cus, q); }, GAT_ERR_ARG, "null statistics", kNull);
        expect_refusal<StatsPlan>([&](StatsPlan *q) { return stats_plan(&s, B, 0, 2u, kStats, c.cus, q); }, GAT_ERR_ARG, "no blocks per estimate", "blocks_per_estimate must be positive");
        expect_refusal<StatsPlan>([&](StatsPlan *q) { return stats_plan(nullptr, B, bpe, flags | 4u, kStats, c.cus, q); }, GAT_ERR_ARG, "unknown flags", "unknown flags");
        expect_refusal<StatsPlan>([&](StatsPlan *q) { return stats_plan(nullptr, 0, bpe, flags, kStats, c.cus, q); }, GAT_ERR_ARG, "null signal", kNull);
        expect_refusal<StatsPlan>([&](StatsPlan *q) { return stats_plan(&s, 0, bpe, flags, kStats, c.cus, q); }, GAT_ERR_ARG, "no blocks", "num_blocks must be positive");
        expect_desc_refusals<StatsPlan>(s, B, [&](const gat_signal_desc *d, StatsPlan *q) { return stats_plan(d, B, bpe, flags, kStats, c.cus, q); }, "chan_stride must be 0");
    }
    std::printf("planned %ld statistics calls (%ld with 16-byte loads, %ld with split blocks, %ld in several batches)\n", n.calls, n.vec, n.split, n.batched);
    CHECK(n.calls == kSweep && n.vec > kSweep / 5 && n.vec < kSweep * 3 / 5 && n.split > kSweep / 10 && n.batched > kSweep / 10, "the statistics sweep lost its balance");
}

void sweep_st_cov_plans(std::mt19937_64 &rng)
{
    const char *const chan = "chan_stride must be 0 (one signal, one covariance)", *const sizes = "num_blocks and blocks_per_estimate must be positive";
    Tally n;
    long tapped = 0;
    for (int it = 0; it < kSweep; ++it) {
        const Call c = random_call(rng, it, true);
        const gat_signal_desc &s = c.sig;
        const int M = s.num_ants, B = c.B, bpe = c.bpe, T = c.T, Q = M * T;
        StCovPlan p;
        poison(&p);
        const Refusal r = st_cov_plan(&s, B, bpe, T, kCov, kCov, c.cus, &p);
        CHECK(r.code == GAT_OK, "space-time covariance: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++n.calls, tapped += T > 1;
        const EstimatePlan &e = p.est;
        const long long chunk = st_cov_geom(M, T).chunk;
        CHECK(p.Q == Q && e.B == B && e.bpe == bpe && e.round_to == chunk && e.min_seg == 8 * chunk && e.workgroups_wanted == (long long)c.cus * 4 &&
                  e.slice_bytes == (size_t)8 * Q * Q && e.cap_bytes == kStCovScratchCap,
              "space-time covariance: the rule of M %d T %d", M, T);
        // snapshot n of a block is samples n .. n + T - 1, newest last: the last snapshot's newest sample is the block's last
        CHECK(e.N == s.num_samples - T + 1 && e.N >= 1 && (e.N - 1) + (T - 1) == s.num_samples - 1, "space-time covariance: %lld snapshots of %lld samples, %d taps", e.N, (long long)s.num_samples, T);
        walk_cut_cap(rng, it, e, 1, 0, &n, "space-time covariance");

        // the refusals, each from this valid call, in the entry point's order
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(nullptr, 0, bpe, T, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "null signal", kNull);
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&s, B, 0, T, nullptr, kCov, c.cus, q); }, GAT_ERR_ARG, "null cov_re", kNull);
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&s, B, bpe, T, kCov, nullptr, c.cus, q); }, GAT_ERR_ARG, "null cov_im", kNull);
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&s, 0, bpe, 0, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "no blocks", sizes);
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&s, B, 0, T, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "no blocks per estimate", sizes);
        gat_signal_desc t = s;
        t.layout = 4;
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&t, B, bpe, 0, kCov, kCov, c.cus, q); }, GAT_ERR_RANGE, "no taps", "num_taps outside 1 .. 16");
        expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&s, B, bpe, GAT_MAX_ST_TAPS + 1, kCov, kCov, c.cus, q); }, GAT_ERR_RANGE, "too many taps", "num_taps outside 1 .. 16");
        expect_desc_refusals<StCovPlan>(s, B, [&](const gat_signal_desc *d, StCovPlan *q) { return st_cov_plan(d, B, bpe, T, kCov, kCov, c.cus, q); }, chan);
        t = s, t.num_ants = GAT_MAX_ARRAY_ANTS / T + 1;
        if (t.num_ants <= GAT_MAX_ARRAY_ANTS)
            expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&t, B, bpe, T, kCov, kCov, c.cus, q); }, GAT_ERR_RANGE, "num_ants * num_taps above 64", "num_ants * num_taps above 64");
        if (T > 1) {
            t = s, t.num_samples = T - 1;
            expect_refusal<StCovPlan>([&](StCovPlan *q) { return st_cov_plan(&t, B, bpe, T, kCov, kCov, c.cus, q); }, GAT_ERR_ARG, "a block shorter than the delay line");
        }
    }
    std::printf("planned %ld space-time covariance calls (%ld of several taps, %ld with split blocks, %ld in several batches)\n", n.calls, tapped, n.split, n.batched);
    CHECK(n.calls == kSweep && tapped > kSweep * 4 / 5 && n.split > kSweep / 10 && n.batched > kSweep / 10, "the space-time covariance sweep lost its balance");
}

// ---- the pinned regimes: the arithmetic that tests/test_array_domain_gpu.py states, as literal numbers, for every device size ----
struct Launch {
    int e0, en, b0, bn;
    long long G, splits, seg_len;
};
// plans an aligned (tidy) or off-by-one-sample covariance call and returns its launches (at most 4 are kept)
int cov_launches(int layout, int M, long long N, int B, int bpe, bool tidy, int cus, bool *vec, Launch (&out)[4])
{
    const long long bs = (N + 7) / 8 * 8;
    const uintptr_t off = tidy ? 0 : (uintptr_t)layout_sample_bytes(layout);
    const gat_signal_desc s = desc(0x100000000ull + off, 0x4000000000ull + off, layout, M, N, bs * B, bs);
    CovPlan p{};
    const Refusal r = cov_plan(&s, B, bpe, kCov, kCov, cus, &p);
    CHECK(r.code == GAT_OK, "pinned: a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
    if (r.code != GAT_OK) return 0;
    *vec = p.vec;
    int n = 0;
    for (EstimateLaunches t(p.est); t.next(); ++n)
        if (n < 4) out[n] = {t.e0, t.en, t.b0, t.bn, t.G, t.splits, t.seg_len};
    return n;
}

void pinned_regimes()
{
    Launch l[4] = {};
    bool vec = false;
    for (int cus : kCus) {
        // tiled, B = 5, bpe = 3: N / min_seg binds
        const struct { int M; long long N; int chunk; long long seg_len, splits, G; } tiled[] = {{9, 9000, 255, 2295, 4, 12}, {33, 3000, 88, 792, 4, 12}, {64, 1000, 24, 216, 5, 15}};
        for (const auto &c : tiled)
            for (int layout = 0; layout < 4; ++layout) {
                CHECK(cov_tile_geom(c.M).chunk == c.chunk, "pinned: chunk %d at M %d", cov_tile_geom(c.M).chunk, c.M);
                const int n = cov_launches(layout, c.M, c.N, 5, 3, true, cus, &vec, l);
                CHECK(n == 1 && !vec && l[0].en == 2 && l[0].bn == 5 && l[0].seg_len == c.seg_len && l[0].splits == c.splits && l[0].G == c.G,
                      "pinned: tiled M %d N %lld on %d CUs: %d launches, seg_len %lld splits %lld G %lld", c.M, c.N, cus, n, l[0].seg_len, l[0].splits, l[0].G);
            }
        // streaming, N = 3072 v + 777, B = 5, bpe = 3
        for (int M : {1, 5, 8})
            for (int layout = 0; layout < 4; ++layout) {
                const long long v = layout_vec_samples(layout);
                const int n = cov_launches(layout, M, 3072 * v + 777, 5, 3, true, cus, &vec, l);
                CHECK(n == 1 && vec && l[0].en == 2 && l[0].splits == 3 && l[0].seg_len == 1280 * v && l[0].G == 9,
                      "pinned: streaming M %d layout %d on %d CUs: %d launches, seg_len %lld splits %lld G %lld", M, layout, cus, n, l[0].seg_len, l[0].splits, l[0].G);
            }
        // more units than workgroups: 5000 blocks of 37 samples in one estimate, G = per_est = every workgroup the launch wants
        for (int M : {4, 16})
            for (int tidy = 0; tidy < 2; ++tidy) {
                const int n = cov_launches(0, M, 37, 5000, 5000, tidy != 0, cus, &vec, l);
                const long long per_est = (long long)cus * (vec ? 8 : 4);
                CHECK(n == 1 && vec == (M == 4 && tidy) && l[0].en == 1 && l[0].splits == 1 && l[0].G == per_est, "pinned: 5000 blocks, M %d on %d CUs: G %lld of %lld", M, cus, l[0].G, per_est);
            }
        // more estimates than workgroups: one workgroup an estimate
        for (int bpe : {1, 3})
            for (int M : {4, 16}) {
                const int B = bpe == 1 ? 5003 : 15001, E = bpe == 1 ? 5003 : 5001;
                const int n = cov_launches(2, M, 12, B, bpe, true, cus, &vec, l);
                CHECK(n == 1 && l[0].en == E && l[0].bn == B && l[0].splits == 1 && l[0].G == 1, "pinned: %d estimates, M %d on %d CUs: G %lld", E, M, cus, l[0].G);
            }
        // the batches at their two bounds: 256 MB of 32 KB slices, and the clamp to 2^20 estimates
        int n = cov_launches(1, 64, 3, 8192 + 5, 1, true, cus, &vec, l);
        CHECK(n == 2 && l[0].e0 == 0 && l[0].en == 8192 && l[0].b0 == 0 && l[0].bn == 8192 && l[1].e0 == 8192 && l[1].en == 5 && l[1].b0 == 8192 && l[1].bn == 5 && l[0].G == 1 && l[1].G == 1,
              "pinned: 8192 + 5 estimates of 64 antennas on %d CUs: %d launches, %d and %d", cus, n, l[0].en, l[1].en);
        n = cov_launches(0, 1, 4, (1 << 20) + 3, 1, true, cus, &vec, l);
        CHECK(n == 2 && l[0].e0 == 0 && l[0].en == 1 << 20 && l[0].bn == 1 << 20 && l[1].e0 == 1 << 20 && l[1].en == 3 && l[1].b0 == 1 << 20 && l[1].bn == 3 && l[0].G == 1 && l[1].G == 1,
              "pinned: 2^20 + 3 estimates of one antenna on %d CUs: %d launches, %d and %d", cus, n, l[0].en, l[1].en);
    }
    std::printf("pinned the covariance's regimes for %zu device sizes\n", sizeof kCus / sizeof kCus[0]);
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261020);
    pinned_regimes();
    sweep_estimate_splits(rng);
    sweep_cov_plans(rng);
    sweep_stats_plans(rng);
    sweep_st_cov_plans(rng);
    std::printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
