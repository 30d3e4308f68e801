// main.cpp -- drives libgat's C ABI (the real gat_api.cpp, gat_planner.cpp, gat_group.cpp, gat_resident_api.cpp, gat_acq_api.cpp,
// gat_array_api.cpp, gat_codes.cpp and gat_version.cpp) on the host-only stand-ins of
// this directory, under AddressSanitizer + UndefinedBehaviorSanitizer:
//   1. thousands of random correlate calls on L1 / L5 and random caller's tables (formats, alignments, ragged lengths, strides, tap lists, flags, options) -- every
//      launch the planner emits is checked against the kernel's contract by fake_kernels.cpp; error paths must return
//      GAT_ERR_* codes, never crash;
//   2. the closed loop (eager and graph replay with its LRU), device groups (shard, replicate, correlate, gather), the
//      stand-alone operators, timers, scratch reallocation;
//   1a. a fixed grid of caller's code tables (1 .. 120 000 chips, +-1 or not) under the default options: every valid call launches;
//   1c. a fixed grid of tap lists (the GPU tests' lists and permutations of them) by layout, antennas, channels and kernel
//      selection: every valid call launches, with the launches the sorted taps' grouping asks for, covering every tap once;
//   1b. random acquisition searches (gat_acq_api.cpp): valid and invalid configs, L1 / L5 tables, caller's grid or none --
//      every launch is checked by fake_kernels.cpp, which touches every byte the kernels would; the host statistics on grids with ties;
//   1d. random antenna-array calls (gat_array_api.cpp): covariances of every layout, antenna count, alignment and work split on
//      simulated devices of 64 .. 512 CUs -- every (block, sample) must be read exactly once, the outputs written whole and
//      nothing else --, refusals with their documented status and no launch, the estimate batch loop; weights, beamforming,
//      the weighted update and the weighted native run (eager and graph);
//   3. the resident correlator's host side against a host thread that plays the device: rings at random distances around
//      the kernel's idle limit and call budget, park, code-table change, free, close, destroy with correlators still open --
//      every call must return exactly what the emulated workgroups posted, summed by the host's second stage.
// Exit code 0: no sanitizer report, no broken invariant, no wrong result.   usage: hostsim [calls] [seed]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <thread>
#include <vector>

#include "gat.h"
#include "gat_array_kernels.h"
#include "gat_ctx.h"
#include "gat_internal.h"
#include "hostsim.h"

static int failures = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++failures;                                     \
            std::fprintf(stderr, "FAILED: %s -- ", #cond);  \
            std::fprintf(stderr, __VA_ARGS__);              \
            std::fprintf(stderr, "\n");                     \
        }                                                   \
    } while (0)

static std::mt19937_64 rng;
static long long uni(long long lo, long long hi) { return std::uniform_int_distribution<long long>(lo, hi)(rng); }
static double unif(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); }
template <class T> static T pick(std::initializer_list<T> l) { return *(l.begin() + uni(0, (long long)l.size() - 1)); }

// bytes of one sample in one plane and samples of one 16-byte load, by layout: the library's arithmetic (gat_internal.h), pinned here
using gat::layout_sample_bytes;
using gat::layout_vec_samples;
static_assert(layout_sample_bytes(0) == 4 && layout_sample_bytes(1) == 8 && layout_sample_bytes(2) == 4 && layout_sample_bytes(3) == 2, "bytes per sample");
static_assert(layout_vec_samples(0) == 4 && layout_vec_samples(1) == 2 && layout_vec_samples(2) == 4 && layout_vec_samples(3) == 8, "samples per load");

// A caller's chip table (gat_set_codes takes any int8 chips, 1 .. 120 000 per row), [Lc x P] column-major.  kind 0: random
// +-1; 1: +-1 with some chips 0; 2: {-1, 0, +1}; 3: the whole int8 range, -128 and 127 included.
static std::vector<int8_t> chip_table(int Lc, int P, int kind)
{
    std::vector<int8_t> t((size_t)Lc * P);
    for (auto &v : t) v = kind == 3 ? (int8_t)uni(-128, 127) : kind == 2 ? (int8_t)uni(-1, 1) : (int8_t)(uni(0, 1) ? 1 : -1);
    if (kind == 1)
        for (int i = 0; i < std::max(1, Lc / 50); ++i) t[(size_t)uni(0, (long long)t.size() - 1)] = 0;
    return t;
}
static bool all_pm1(const std::vector<int8_t> &t) { return gat::codes_all_pm1(t.data(), (int)t.size(), 1); }
// the one refusal a correlate call with valid records may meet: the code-span bound (gat_chan_rules.h), evaluated here
static bool span_refused(const std::vector<gat_channel_params> &prm, double fs, long long N, const std::vector<int32_t> &sh, int Lc)
{
    long long ms = 0;
    for (int32_t s : sh) ms = std::max<long long>(ms, std::llabs((long long)s));
    for (const auto &p : prm)
        if (gat::code_span_bad(p.code_freq_hz / fs, p.code_phase_chips, (double)(N + ms), Lc)) return true;
    return false;
}

// After a call: the launches of the correlator wrote every position of the caller's tap list exactly once, each with the
// caller's shift at that position (tap_index), and a tail launch took the list in the caller's order.
static bool taps_covered(const std::vector<int32_t> &sh, const char *what)
{
    const auto &cv = hostsim::tap_cover;
    std::vector<int> seen(sh.size(), 0);
    bool ok = !cv.main.empty();
    for (const auto &is : cv.main) {
        const bool in = is.first >= 0 && is.first < (int)sh.size() && sh[is.first] == is.second;
        ok &= in;
        if (in) ++seen[is.first];
    }
    for (int n : seen) ok &= n == 1;
    for (const auto &t : cv.tail) ok &= t == std::vector<int>(sh.begin(), sh.end());
    EXPECT(ok, "%s: %zu tap launches entries, %zu tails for %zu taps", what, cv.main.size(), cv.tail.size(), sh.size());
    return ok;
}

// Sorted taps cut greedily into groups of <= kMaxTapsPerLaunch within kMaxLaunchSpan of the group's first tap: the vector
// kernel's launches of one call.
static long greedy_groups(std::vector<int32_t> sh)
{
    std::sort(sh.begin(), sh.end());
    long n = 0;
    for (size_t t0 = 0; t0 < sh.size(); ++n) {
        size_t t1 = t0 + 1;
        while (t1 < sh.size() && t1 - t0 < (size_t)gat::kMaxTapsPerLaunch && (long long)sh[t1] - sh[t0] <= gat::kMaxLaunchSpan) ++t1;
        t0 = t1;
    }
    return n;
}

// The tap lists of tests/test_tap_domain_gpu.py for a block of N samples (one tap at 0, before and after the block; order and
// duplicates; the count and span boundaries of a launch; the matrix kernels' limits; N + max|shift| = 2^30 - 1).
static std::vector<std::vector<int32_t>> tap_lists(int N)
{
    std::vector<std::vector<int32_t>> T;
    const int32_t far = (1 << 30) - 1 - N;
    auto shuffled = [](std::vector<int32_t> v) { std::shuffle(v.begin(), v.end(), rng); return v; };
    auto range = [](int lo, int hi, int step) { std::vector<int32_t> v; for (int x = lo; x < hi; ++x) v.push_back(x * step); return v; };
    T.push_back({0});
    T.push_back({-N - 5});
    T.push_back({3 * N});
    T.push_back({1, 0, -1});
    {
        std::vector<int32_t> v = range(-100, 101, 1);
        v = shuffled(v);
        v.resize(32);
        T.push_back(v);
        T.push_back(std::vector<int32_t>(32, 7));
        std::vector<int32_t> p = shuffled(range(-60, 61, 1));
        p.resize(16);
        std::vector<int32_t> d = p;
        for (int32_t x : shuffled(p)) d.push_back(x);
        T.push_back(d);
    }
    T.push_back(range(-4, 4, 3));
    T.push_back(shuffled(range(-4, 5, 3)));
    T.push_back(shuffled(range(-8, 9, 1)));
    {
        std::vector<int32_t> v = range(-4, 5, 11);
        v.push_back(5000);
        T.push_back(shuffled(v));
    }
    auto spread = [&](int L, int s) {
        std::vector<int32_t> d(L);
        for (int l = 0; l < L; ++l) d[l] = (int32_t)std::lround(L > 1 ? (double)s * l / (L - 1) : 0.0);
        const int32_t mid = d[L / 2];
        for (auto &x : d) x -= mid;
        return shuffled(d);
    };
    T.push_back(spread(8, 769));
    T.push_back(shuffled({far, far - 1, far - 2, far - 7}));
    T.push_back(shuffled({-far, -far + 3, -far + 1}));
    T.push_back({-far, 0, far});
    for (int s : {511, 512, 513, 2047, 2048, 2049}) {
        const int b = -((s / 2) & ~1);
        T.push_back(shuffled({b, b + 2, 0, b + ((s - 2) & ~1), b + s}));
        T.push_back(shuffled({b, b + 1, b + 3, 0, b + s - 1, b + s}));
    }
    for (int L : {6, 7, 8, 11, 16})
        for (int s : {0, 1, 767, 768}) T.push_back(spread(L, s));
    const size_t n = T.size();
    for (size_t i = 0; i < n; ++i) T.push_back(shuffled(T[i])); // and a random permutation of each
    return T;
}

int main(int argc, char **argv)
{
    const int calls = argc > 1 ? std::atoi(argv[1]) : 4000;
    rng.seed(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20260401ull);
    gat_ctx *ctx = nullptr;
    EXPECT(gat_create(0, GAT_OWN_STREAM, &ctx) == GAT_OK, "gat_create");
    std::printf("%s\n", gat_version());

    // correlate before the code table: a state error, not a crash
    {
        gat_signal_desc sig = {(void *)0x100000, (void *)0x200000, GAT_LAYOUT_PLANAR, 1, 1000, 1000, 1000, 0};
        gat_channel_params p = {0, 0, 1.023e6, 0.0, 0.0, 0.0};
        int32_t sh[3] = {-1, 0, 1};
        float o[3];
        EXPECT(gat_downconvert_and_correlate(ctx, &sig, &p, 1, 1, 3, sh, 1e6, o, o, 0) == GAT_ERR_STATE, "correlate without codes");
    }
    int32_t lc = 0;
    double fc = 0.0;
    EXPECT(gat_gen_codes("GPSL1", 0, nullptr, &lc, &fc) == GAT_OK && lc == 1023, "code sizes");
    std::vector<int8_t> codes((size_t)lc * 32);
    EXPECT(gat_gen_codes("GPSL1", 32, codes.data(), &lc, &fc) == GAT_OK, "gen codes");
    EXPECT(gat_set_codes(ctx, codes.data(), lc, 32) == GAT_OK, "set codes");
    int32_t lc5 = 0;
    double fc5 = 0.0;
    gat_gen_codes("GPSL5", 0, nullptr, &lc5, &fc5);
    std::vector<int8_t> codes5((size_t)lc5 * 8);
    EXPECT(gat_gen_codes("GPSL5", 8, codes5.data(), &lc5, &fc5) == GAT_OK, "gen L5 codes");

    // ---- 1. random correlate calls ---------------------------------------------------------------------------------------
    const char *opts[] = {"sync_flag_wgs", "max_ant_tile", "dc_aw", "dc_kt", "dc_bpw", "dc_bpw_force", "dc_wgs_per_cu", "dc_one_wave",
                          "dc_one_wave_min", "dc_ow_seg", "dc_depth", "dc_keep_l2", "dc_align", "dc_aw2", "dc_seg", "dc_bits", "dc_quads", "mc_i16_terms"};
    const long long opt_lo[] = {0, 1, 1, 1, 1, 0, 0, 0, -1, 1, 1, -1, 0, -1, 0, 0, -1, 2}, opt_hi[] = {2048, 4, 4, 4, 64, 8, 16, 1, 64, 8, 2, 1, 1, 1, 8, 2, 1, 3};
    EXPECT(gat_set_option(ctx, "no_such_option", 1) == GAT_ERR_ARG && gat_set_option(ctx, "dc_depth", 7) == GAT_ERR_RANGE, "option errors");
    EXPECT(gat_set_matrix_core(ctx, 7) != GAT_OK, "kernel selection: bad mode");
    long ok_calls = 0, rejected = 0;
    long tables_bound = 0, long_int8_calls = 0, valid_refused = 0; // (caller's tables: bound, calls on long ones not +-1, valid calls refused)
    int tbl_which = 0, tbl_P = 32, tbl_Lc = lc; // 0 L1, 1 L5, 2 a caller's table
    double tbl_fc = fc;
    bool tbl_int8 = false;
    std::vector<int8_t> caller;
    for (int it = 0; it < calls; ++it) {
        if (it % 47 == 0) { // a dual-frequency receiver alternates tables on one context -- and now and then a caller's own
            tbl_which = (tbl_which + 1) % 3;
            if (tbl_which == 2) {
                const int len = (int)pick<long long>({uni(1, 40), uni(1, 2100), uni(2000, 20000), uni(20000, 120000), 120000, 1023, 10230});
                const int kind = (int)uni(0, 3);
                tbl_P = (int)uni(1, 64);
                caller = chip_table(len, tbl_P, kind);
                tbl_Lc = len, tbl_fc = pick<double>({1.023e6, 10.23e6, 0.5e6}), tbl_int8 = !all_pm1(caller);
                EXPECT(gat_set_codes(ctx, caller.data(), len, tbl_P) == GAT_OK, "bind a caller's table (%d chips, kind %d, %d PRNs)", len, kind, tbl_P);
                ++tables_bound;
            } else {
                tbl_P = tbl_which ? 8 : 32, tbl_Lc = tbl_which ? lc5 : lc, tbl_fc = tbl_which ? fc5 : fc, tbl_int8 = false;
                EXPECT((tbl_which ? gat_set_codes(ctx, codes5.data(), lc5, 8) : gat_set_codes(ctx, codes.data(), lc, 32)) == GAT_OK, "rebind codes");
            }
        }
        if (it % 13 == 0) EXPECT(gat_set_matrix_core(ctx, (int32_t)uni(0, 3)) == GAT_OK, "kernel selection");
        if (it % 11 == 0) {
            const int o = (int)uni(0, (long long)(sizeof(opts) / sizeof(opts[0])) - 1);
            EXPECT(gat_set_option(ctx, opts[o], uni(opt_lo[o], opt_hi[o])) == GAT_OK, "option %s", opts[o]);
        }
        const int fmt = (int)uni(0, 3), M = (int)pick<long long>({1, 1, 2, 3, 4, 4, 5, 8, 12, 16, 16, 20, 32, 48, 64, 128});
        const int K = (int)pick<long long>({1, 1, 1, 2, 3, 4, 5, 8, 12, 16, 24, 32, 64});
        const int B = M * K >= 256 ? (int)pick<long long>({1, 1, 2, 3}) : (int)pick<long long>({1, 1, 1, 2, 3, 7, 16, 64, 500});
        const int L = (int)pick<long long>({1, 2, 3, 3, 5, 7, 8, 11, 17, 32});
        long long N = pick<long long>({uni(1, 64), uni(64, 5000), 2048, 2500, 4096, 20000, 50000, uni(5000, 300000), 262144});
        if (uni(0, 3) == 0) N -= N % layout_vec_samples(fmt);
        if (N < 1) N = layout_vec_samples(fmt);
        const long long pad = pick<long long>({0, 0, 0, layout_vec_samples(fmt), 1, 3, 32});
        long long bstride = N + pad, astride = bstride * B + pick<long long>({0, 0, layout_vec_samples(fmt) * 4, 1});
        const long long cstride = (K > 1 && uni(0, 5) == 0) ? astride * M : 0;
        const uintptr_t mis = pick<long long>({0, 0, 0, 0, 4, 8, 2});
        gat_signal_desc sig = {(void *)(uintptr_t)(0x10000000 + mis), fmt == 0 ? (void *)(uintptr_t)(0x50000000 + mis) : nullptr, fmt, M, N, astride, bstride, cstride};
        std::vector<int32_t> sh(L);
        const int spread = (int)pick<long long>({1, 2, 10, 128, 400, 700, 1500, 5000});
        for (int l = 0; l < L; ++l) sh[l] = (int32_t)uni(-spread, spread);
        if (uni(0, 1)) std::sort(sh.begin(), sh.end());
        const double fs = N / 1e-3;
        const int P = tbl_P, Lc = tbl_Lc;
        std::vector<gat_channel_params> prm((size_t)B * K);
        for (auto &p : prm) p = {(int32_t)uni(0, P - 1), 0, tbl_fc * (1 + unif(-1e-5, 1e-5)), unif(-5e3, 5e3), unif(0, Lc), unif(0, 1)};
        const int bad = (int)uni(0, 40); // now and then something the validation must catch
        if (bad == 0) prm[0].prn = P + 3;
        if (bad == 1) prm.back().code_phase_chips = NAN;
        if (bad == 2) prm[0].code_freq_hz = -1.0;
        const uint32_t flags = uni(0, 6) == 0 ? GAT_FLAG_ATOMIC : 0u;
        const size_t outs = (size_t)B * K * L * M;
        void *o_re = nullptr, *o_im = nullptr, *prm_dev = nullptr;
        gat_malloc(ctx, outs * sizeof(float), &o_re);
        gat_malloc(ctx, outs * sizeof(float), &o_im);
        int32_t rc;
        if (uni(0, 1)) {
            hostsim::tap_cover.clear();
            rc = gat_downconvert_and_correlate(ctx, &sig, prm.data(), B, K, L, sh.data(), fs, (float *)o_re, (float *)o_im, flags);
            if (rc == GAT_OK) taps_covered(sh, "random sweep, host records");
            EXPECT(rc == GAT_OK || rc == GAT_ERR_RANGE || rc == GAT_ERR_ARG, "host-parameter call: %d (%s)", rc, gat_last_error(ctx));
            EXPECT(bad > 2 || rc != GAT_OK, "a bad record passed the validation (case %d)", bad);
        } else {
            gat_malloc(ctx, prm.size() * sizeof(gat_channel_params), &prm_dev);
            gat_memcpy_h2d(ctx, prm_dev, prm.data(), prm.size() * sizeof(gat_channel_params));
            const uint32_t graph = uni(0, 3) == 0 && !flags ? GAT_FLAG_GRAPH : 0u;
            hostsim::tap_cover.clear();
            rc = gat_downconvert_and_correlate_dev(ctx, &sig, (gat_channel_params *)prm_dev, B, K, L, sh.data(), fs, (float *)o_re, (float *)o_im,
                                                   flags | graph);
            if (rc == GAT_OK && !graph) taps_covered(sh, "random sweep, device records"); // (a replayed graph launches nothing here)
            EXPECT(rc == GAT_OK || rc == GAT_ERR_RANGE || rc == GAT_ERR_ARG, "device-parameter call: %d (%s)", rc, gat_last_error(ctx));
        }
        // a valid call launches -- or meets the code-span bound; the planner refuses nothing (whatever the table and options)
        if (bad > 2) {
            const bool ok = rc == GAT_OK || (rc == GAT_ERR_RANGE && span_refused(prm, fs, N, sh, Lc));
            EXPECT(ok, "valid call refused: %d (%s): table %d (%d chips, %d PRNs%s), layout %d M %d K %d L %d B %lld N %lld", rc, gat_last_error(ctx), tbl_which, Lc, P,
                   tbl_int8 ? ", int8" : "", fmt, M, K, L, (long long)B, N);
            valid_refused += !ok;
            long_int8_calls += tbl_int8 && Lc >= 20000;
        }
        if (rc == GAT_OK) {
            ++ok_calls;
            gat_launch_info li;
            EXPECT(gat_last_launch_info(ctx, &li, sizeof li) == GAT_OK && li.workgroups > 0 && (li.vec == 4 || li.vec == 1), "launch info");
            const bool aligned = mis % 16 == 0 && (M == 1 || astride % layout_vec_samples(fmt) == 0) && (B == 1 || bstride % layout_vec_samples(fmt) == 0) && cstride % layout_vec_samples(fmt) == 0;
            EXPECT((li.vec == 4) == (aligned && N * layout_sample_bytes(fmt) < (1ll << 31)), "vector path: vec %d for aligned %d (fmt %d N %lld M %d B %d)", li.vec, (int)aligned, fmt, N, M, B);
        } else {
            ++rejected;
        }
        EXPECT(gat_sync(ctx) == GAT_OK, "sync");
        gat_free(ctx, o_re);
        gat_free(ctx, o_im);
        if (prm_dev) gat_free(ctx, prm_dev);
    }
    std::printf("correlate sweep: %ld calls planned and launched, %ld rejected by validation; %ld vector launches, %ld matrix-core launches, %ld second stages, %ld tails, %ld graphs (%ld replays)\n",
                ok_calls, rejected, hostsim::counters.dc_launches.load(), hostsim::counters.mfma_launches.load(), hostsim::counters.finalize_launches.load(), hostsim::counters.tail_launches.load(),
                hostsim::counters.graphs.load(), hostsim::counters.graph_launches.load());
    EXPECT(ok_calls > calls / 2 && hostsim::counters.tail_launches > 0 && hostsim::counters.finalize_launches > 0 && (calls < 500 || hostsim::counters.mfma_launches > 0),
           "the sweep covers second stages, tails and the matrix-core kernels");
    EXPECT(gat_set_matrix_core(ctx, 1) == GAT_OK, "kernel selection back to auto");
    for (int o = 0; o < 18; ++o) gat_set_option(ctx, opts[o], o == 17 ? 2 : o == 0 ? 1024 : o == 1 ? 4 : o == 2 ? 4 : o == 3 ? 4 : o == 4 ? 16 : o == 5 ? 0 : o == 6 ? 0 : o == 7 ? 1 : o == 8 ? -1 : o == 9 ? 4 : o == 10 ? 2 : o == 11 ? -1 : o == 12 ? 1 : o == 13 ? -1 : o == 15 ? 1 : o == 16 ? -1 : 0);
    EXPECT(gat_set_codes(ctx, codes.data(), lc, 32) == GAT_OK, "rebind L1");

    // ---- 1a. a fixed grid of caller's tables under the default options ----------------------------------------------------
    // Table lengths from one chip to the 120 000-chip limit, +-1 (sign-bit rows where long) and +-1 with one chip 0 (int8 rows
    // whatever the length: LDS budget, the 2 x 2 tile's fit), by taps, channels, antennas, blocks and layouts.  Every call is
    // valid: it must launch, or meet the code-span bound.
    {
        gat_ctx *tctx = nullptr; // a new context: the library's default options
        EXPECT(gat_create(0, GAT_OWN_STREAM, &tctx) == GAT_OK, "context for the table grid");
        const int lens[] = {1, 7, 16, 33, 511, 2046, 2048, 4092, 5115, 10230, 20000, 30000, 65536, 100000, 120000};
        const int Ls[] = {1, 3, 7}, Ks[] = {1, 2, 3, 4, 8}, Ms[] = {1, 2, 4, 8, 16, 32}, Bs[] = {1, 16, 256};
        const int P = 4;
        const long long N = 20000;
        const double fs = 20e6;
        void *o_re = nullptr, *o_im = nullptr;
        const size_t outs = (size_t)256 * 8 * 7 * 32;
        gat_malloc(tctx, outs * sizeof(float), &o_re);
        gat_malloc(tctx, outs * sizeof(float), &o_im);
        long grid_calls = 0, grid_refused = 0;
        for (int len : lens)
            for (int zero = 0; zero < 2; ++zero) {
                std::vector<int8_t> t = chip_table(len, P, 0);
                if (zero) t[(size_t)uni(0, (long long)t.size() - 1)] = 0;
                EXPECT(gat_set_codes(tctx, t.data(), len, P) == GAT_OK, "bind %d chips", len);
                ++tables_bound;
                for (int L : Ls)
                    for (int K : Ks)
                        for (int M : Ms)
                            for (int B : Bs)
                                for (int fmt = 0; fmt < 4; ++fmt) {
                                    std::vector<int32_t> sh(L);
                                    for (int l = 0; l < L; ++l) sh[l] = l - L / 2;
                                    gat_signal_desc sig = {(void *)(uintptr_t)0x10000000, fmt == 0 ? (void *)(uintptr_t)0x50000000 : nullptr, fmt, M, N, N * B, N, 0};
                                    std::vector<gat_channel_params> prm((size_t)B * K);
                                    for (size_t i = 0; i < prm.size(); ++i)
                                        prm[i] = {(int32_t)(i % P), 0, 1.023e6 * (1 + unif(-1e-5, 1e-5)), unif(-5e3, 5e3), unif(0, len), unif(0, 1)};
                                    const int32_t rc = gat_downconvert_and_correlate(tctx, &sig, prm.data(), B, K, L, sh.data(), fs, (float *)o_re, (float *)o_im, 0);
                                    const bool ok = rc == GAT_OK || (rc == GAT_ERR_RANGE && span_refused(prm, fs, N, sh, len));
                                    EXPECT(ok, "table grid: %d (%s): %d chips%s, layout %d M %d K %d L %d B %d", rc, gat_last_error(tctx), len, zero ? " (one chip 0)" : "", fmt, M, K, L, B);
                                    ++grid_calls;
                                    grid_refused += !ok;
                                    long_int8_calls += zero && len >= 20000;
                                    EXPECT(gat_sync(tctx) == GAT_OK, "sync");
                                }
            }
        gat_free(tctx, o_re);
        gat_free(tctx, o_im);
        EXPECT(gat_destroy(tctx) == GAT_OK, "destroy");
        valid_refused += grid_refused;
        std::printf("code tables: %ld tables bound, %ld grid calls, %ld calls on int8 tables of >= 20000 chips, %ld valid calls refused\n", tables_bound, grid_calls,
                    long_int8_calls, valid_refused);
    }

    // ---- 1c. a fixed grid of tap lists under the default options ------------------------------------------------------------
    // The tap lists of the GPU tests (and a random permutation of each) by layout, antennas, channels and kernel selection: every
    // valid call launches (or meets the code-span bound); the vector kernel runs as many launches as the greedy grouping of the
    // sorted taps; the matrix kernels only within L <= 16 and a span of 768; the launches cover the caller's taps exactly once.
    {
        gat_ctx *tctx = nullptr;
        EXPECT(gat_create(0, GAT_OWN_STREAM, &tctx) == GAT_OK, "context for the tap grid");
        EXPECT(gat_set_codes(tctx, codes.data(), lc, 32) == GAT_OK, "bind L1 for the tap grid");
        const int N = 4096;
        const double fs = 16.368e6;
        const auto lists = tap_lists(N);
        const int Ms[] = {1, 4, 16, 64}, Ks[] = {1, 2, 5};
        void *o_re = nullptr, *o_im = nullptr;
        const size_t outs = (size_t)5 * 32 * 64;
        gat_malloc(tctx, outs * sizeof(float), &o_re);
        gat_malloc(tctx, outs * sizeof(float), &o_im);
        long tap_calls = 0, tap_launches = 0, tap_refused = 0;
        for (int mode = 0; mode < 4; ++mode) {
            EXPECT(gat_set_matrix_core(tctx, mode) == GAT_OK, "kernel selection %d", mode);
            for (const auto &sh : lists)
                for (int fmt = 0; fmt < 4; ++fmt)
                    for (int M : Ms)
                        for (int K : Ks) {
                            const int L = (int)sh.size();
                            gat_signal_desc sig = {(void *)(uintptr_t)0x10000000, fmt == 0 ? (void *)(uintptr_t)0x50000000 : nullptr, fmt, M, N, N, N, 0};
                            std::vector<gat_channel_params> prm((size_t)K);
                            for (int k = 0; k < K; ++k) prm[k] = {k % 32, 0, 1.023e6 * (1 + unif(-1e-5, 1e-5)), unif(-5e3, 5e3), unif(0, lc), unif(0, 1)};
                            const long dc0 = hostsim::counters.dc_launches, mc0 = hostsim::counters.mfma_launches;
                            hostsim::tap_cover.clear();
                            const int32_t rc = gat_downconvert_and_correlate(tctx, &sig, prm.data(), 1, K, L, sh.data(), fs, (float *)o_re, (float *)o_im, 0);
                            const bool ok = rc == GAT_OK || (rc == GAT_ERR_RANGE && span_refused(prm, fs, N, sh, lc));
                            EXPECT(ok, "tap grid: %d (%s): mode %d layout %d M %d K %d L %d", rc, gat_last_error(tctx), mode, fmt, M, K, L);
                            ++tap_calls;
                            tap_refused += !ok;
                            if (rc == GAT_OK) {
                                const long dc = hostsim::counters.dc_launches - dc0, mc = hostsim::counters.mfma_launches - mc0;
                                const long span = (long)*std::max_element(sh.begin(), sh.end()) - *std::min_element(sh.begin(), sh.end());
                                EXPECT((mc == 0 && dc == greedy_groups(sh)) || (mc == 1 && dc == 0 && L <= gat::kMfmaMaxTaps && span <= gat::kMfmaMaxSpan),
                                       "tap grid: %ld vector / %ld matrix-core launches for L %d span %ld (greedy %ld): mode %d layout %d M %d K %d", dc, mc, L, span,
                                       greedy_groups(sh), mode, fmt, M, K);
                                taps_covered(sh, "tap grid");
                                tap_launches += dc + mc;
                            }
                            EXPECT(gat_sync(tctx) == GAT_OK, "sync");
                        }
        }
        gat_free(tctx, o_re);
        gat_free(tctx, o_im);
        EXPECT(gat_destroy(tctx) == GAT_OK, "destroy");
        std::printf("tap grid: %ld calls, %ld tap launches, %ld valid calls refused\n", tap_calls, tap_launches, tap_refused);
    }

    // ---- 1b. random acquisition searches (gat_acquire, gat_acq_stats_host) ---------------------------------------------------
    {
        gat_ctx *fresh = nullptr;
        EXPECT(gat_create(0, GAT_OWN_STREAM, &fresh) == GAT_OK, "context for the state check");
        gat_signal_desc sig = {(void *)0x100000, (void *)0x200000, GAT_LAYOUT_PLANAR, 1, 1000, 1000, 1000, 0};
        gat_acq_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.num_doppler_bins = cfg.num_code_bins = cfg.code_step_samples = 1;
        cfg.code_freq_hz = fc;
        int32_t prn = 0;
        gat_acq_result r{};
        EXPECT(gat_acquire(fresh, &sig, 1, &prn, 1, 4e6, &cfg, nullptr, &r) == GAT_ERR_STATE, "acquire without codes");
        EXPECT(gat_destroy(fresh) == GAT_OK, "destroy");
    }
    long acq_launched = 0, acq_rejected = 0, acq_stats_ok = 0;
    const long acq_split0 = hostsim::counters.acq_split_launches.load();
    gat_ctx *actx = ctx;
    for (int it = 0; it < calls / 4; ++it) {
        const bool l5a = it % 2 == 1;
        const int tbl = l5a ? 8 : 32, Lc = l5a ? lc5 : lc;
        const double fcode = l5a ? fc5 : fc;
        // every other search on a new context: its scratch is then exactly what the call asked for, and ASan sees a carve-up
        // that reaches past it (a reused, larger scratch would hide it)
        if (actx != ctx) EXPECT(gat_destroy(actx) == GAT_OK, "destroy");
        actx = it % 4 < 2 ? ctx : nullptr;
        if (!actx) EXPECT(gat_create(0, GAT_OWN_STREAM, &actx) == GAT_OK, "context for one search");
        EXPECT((l5a ? gat_set_codes(actx, codes5.data(), lc5, 8) : gat_set_codes(actx, codes.data(), lc, 32)) == GAT_OK, "rebind codes");
        const int fmt = (int)uni(0, 3);
        const int M = (int)pick<long long>({1, 1, 2, 3, 4, 7});
        const int B = (int)pick<long long>({1, 1, 2, 3, 5, 9, 40});
        const long long N = pick<int>({0, 1, 2}) == 0 ? uni(1, 300) : uni(1, 12000);
        long long bs = pick<int>({0, 1, 2}) == 0 ? N : pick<int>({0, 1}) ? N + uni(1, 64) : std::max(1ll, N - uni(1, N));
        if (B == 1 && uni(0, 1)) bs = 0;
        const long long as = (B - 1) * bs + N + uni(0, 33);
        const long long extent = (M - 1) * as + (B - 1) * bs + N; // samples the signal spans
        const size_t sbytes = fmt == GAT_LAYOUT_PLANAR ? 4 : fmt == GAT_LAYOUT_INTERLEAVED ? 8 : fmt == GAT_LAYOUT_INTERLEAVED_I16 ? 4 : 2;
        std::vector<unsigned char> sre((size_t)extent * sbytes), sim(fmt == GAT_LAYOUT_PLANAR ? (size_t)extent * sbytes : 0);
        gat_signal_desc sig = {sre.data(), fmt == GAT_LAYOUT_PLANAR ? (void *)sim.data() : nullptr, fmt, M, N, M > 1 ? as : uni(0, 1) * as, bs, 0};
        const double fs = pick<double>({1.5e6, 2.046e6, 4e6, 5e6, 20e6, 20.46e6});
        gat_acq_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.num_doppler_bins = (int)pick<long long>({1, 2, 31, 32, 33, uni(1, 80)});
        cfg.num_code_bins = (int)pick<long long>({1, 255, 256, 257, uni(1, 1200)});
        cfg.code_step_samples = (int)uni(1, 31);
        cfg.if_hz = pick<int>({0, 1}) ? 0.0 : unif(-0.25, 0.25) * fs;
        cfg.code_freq_hz = fcode;
        cfg.doppler_first_hz = unif(-1e4, 0.0);
        cfg.doppler_step_hz = pick<double>({0.0, 250.0, -500.0, 33.3});
        cfg.first_shift = pick<int>({0, 1, 2}) == 0 ? -uni(0, 3 * N) : uni(0, 100000);
        cfg.min_peak_ratio = pick<double>({0.0, 2.0, 2.5});
        cfg.code_length = pick<int>({0, 1}) ? 0 : Lc;
        int P = (int)uni(1, 12);
        std::vector<int32_t> prns((size_t)P);
        for (auto &p : prns) p = (int32_t)uni(0, tbl - 1);
        if (P > 1 && uni(0, 2) == 0) prns[P - 1] = prns[0];
        int blocks = B;
        const gat_signal_desc *sigp = &sig;
        bool bad = true;
        switch (uni(0, 34)) { // one way to be wrong, or none
        case 0: cfg.struct_size = (uint32_t)uni(0, sizeof cfg - 1); break;
        case 1: cfg.reserved = (int32_t)pick<long long>({-1, 1, 7}); break;
        case 2: cfg.code_step_samples = (int)pick<long long>({0, -3, 32, 33, 40}); break;
        case 3: (uni(0, 1) ? cfg.num_doppler_bins : cfg.num_code_bins) = (int)uni(-2, 0); break;
        case 4: P = 0; break;
        case 5: cfg.num_doppler_bins = 4096, cfg.num_code_bins = (int)uni(16385, 40000); break; // above 2^26 bins
        case 6: *pick<double *>({&cfg.if_hz, &cfg.doppler_first_hz, &cfg.doppler_step_hz, &cfg.code_freq_hz, &cfg.min_peak_ratio}) = pick<double>({NAN, INFINITY, -INFINITY}); break;
        case 7: prns[(size_t)uni(0, P - 1)] = (int32_t)pick<long long>({-1, tbl, tbl + 5, 1 << 20}); break;
        case 8: if (M > 1) sig.ant_stride = uni(-5, 0); else sig.num_ants = (int)uni(-1, 0); break;
        case 9: if (B > 1) sig.block_stride = uni(-5, 0); else blocks = (int)uni(-1, 0); break;
        case 10: sig.chan_stride = pick<long long>({1, -1, as}); break;
        case 11: cfg.first_shift = pick<long long>({1ll << 30, -(1ll << 30), 1ll << 40}); break;
        case 12: cfg.code_length = pick<int>({Lc + 1, Lc == lc ? lc5 : lc, -1}); break;
        case 13: sigp = nullptr; break;
        case 14: sig.layout = (int)pick<long long>({-1, 4, 9}); break;
        case 15: sig.im = fmt == GAT_LAYOUT_PLANAR ? nullptr : (void *)sre.data(); break;
        case 16: sig.num_samples = uni(-3, 0); break;
        case 17: cfg.doppler_step_hz = 1e15; break; // carrier beyond every bound
        default: bad = false; break;
        }
        const double fs_call = bad && uni(0, 9) == 0 ? pick<double>({0.0, -1.0, NAN}) : fs;
        if (fs_call != fs) bad = true;
        std::vector<float> power;
        const long long cells = (long long)std::max(P, 0) * std::max(cfg.num_doppler_bins, 0) * std::max(cfg.num_code_bins, 0);
        const bool own = uni(0, 1) == 1 && cells > 0 && cells < (1ll << 24);
        if (own) power.assign((size_t)cells, NAN);
        std::vector<gat_acq_result> res((size_t)std::max(P, 1));
        const int32_t rc = gat_acquire(actx, sigp, blocks, prns.data(), P, fs_call, &cfg, own ? power.data() : nullptr, res.data());
        if (bad) {
            EXPECT(rc == GAT_ERR_ARG || rc == GAT_ERR_RANGE || rc == GAT_ERR_STATE, "acquire: bad config (it %d) returned %d", it, rc);
            ++acq_rejected;
        } else {
            EXPECT(rc == GAT_OK, "acquire: valid config (it %d: layout %d M %d B %d N %lld D %d J %d s %d P %d) returned %d: %s", it, fmt, M, B, N,
                   cfg.num_doppler_bins, cfg.num_code_bins, cfg.code_step_samples, P, rc, gat_last_error(actx));
            if (rc == GAT_OK) {
                ++acq_launched;
                for (int p = 0; p < P; ++p) EXPECT(res[(size_t)p].prn == prns[(size_t)p], "acquire: result %d for prn %d", p, prns[(size_t)p]);
                if (own) EXPECT(std::all_of(power.begin(), power.end(), [](float v) { return v == 0.0f; }), "acquire: the caller's grid not (all) written");
            }
        }
        // the host statistics on a grid with ties (a few integer levels): the peak is the first maximum
        if (cells > 0 && cells < (1ll << 22)) {
            std::vector<float> grid((size_t)cells);
            const int levels = (int)uni(1, 6);
            for (auto &v : grid) v = (float)uni(0, levels);
            std::vector<gat_acq_result> hres((size_t)P);
            const int32_t rs = gat_acq_stats_host(grid.data(), P, cfg.num_doppler_bins, cfg.num_code_bins, &cfg, fs_call, N, hres.data());
            if (bad && rs != GAT_OK) {
                EXPECT(rs == GAT_ERR_ARG || rs == GAT_ERR_RANGE, "stats: returned %d", rs);
            } else if (rs == GAT_OK) {
                ++acq_stats_ok;
                const long long c1 = (long long)cfg.num_doppler_bins * cfg.num_code_bins;
                for (int p = 0; p < P; ++p) {
                    const float *g = grid.data() + (size_t)p * c1;
                    const long long pk = std::max_element(g, g + c1) - g;
                    const gat_acq_result &h = hres[(size_t)p];
                    EXPECT(h.doppler_bin == pk / cfg.num_code_bins && h.code_bin == pk % cfg.num_code_bins && h.peak_power == (double)g[pk],
                           "stats: peak (%d, %d) instead of the first maximum %lld", h.doppler_bin, h.code_bin, pk);
                    EXPECT(h.num_noise_bins >= 0 && h.num_noise_bins < c1 && (h.detected == -1) == (h.num_noise_bins < 64) && h.detected >= -1 && h.detected <= 1,
                           "stats: %lld noise bins, detected %d", (long long)h.num_noise_bins, h.detected);
                }
            } else {
                EXPECT(cfg.code_length == 0 && rs == GAT_ERR_ARG, "stats: a valid config (code_length %d) returned %d", cfg.code_length, rs);
            }
        }
    }
    if (actx != ctx) EXPECT(gat_destroy(actx) == GAT_OK, "destroy");
    {
        int32_t many[1] = {0};
        gat_acq_config cfg{};
        cfg.struct_size = sizeof cfg;
        cfg.num_doppler_bins = cfg.num_code_bins = cfg.code_step_samples = 1;
        cfg.code_freq_hz = fc;
        float g[1] = {1.0f};
        gat_acq_result r{};
        EXPECT(gat_acq_stats_host(nullptr, 1, 1, 1, &cfg, 4e6, 100, &r) == GAT_ERR_ARG && gat_acq_stats_host(g, 1, 1, 1, &cfg, 4e6, 0, &r) == GAT_ERR_ARG &&
                   gat_acq_stats_host(g, 1, 1, 1, &cfg, 4e6, 100, nullptr) == GAT_ERR_ARG && gat_acq_stats_host(g, 1, 1, 1, nullptr, 4e6, 100, &r) == GAT_ERR_ARG,
               "stats: null arguments");
        std::vector<int32_t> lots(70000, 0); // more PRNs than grid z can carry
        std::vector<gat_acq_result> rr(lots.size());
        EXPECT(gat_set_codes(ctx, codes.data(), lc, 32) == GAT_OK, "rebind L1");
        gat_signal_desc sig = {many, nullptr, GAT_LAYOUT_INTERLEAVED_I8, 1, 1, 0, 0, 0};
        EXPECT(gat_acquire(ctx, &sig, 1, lots.data(), (int32_t)lots.size(), 4e6, &cfg, nullptr, rr.data()) == GAT_ERR_RANGE, "acquire: 70000 PRNs");
        ++acq_rejected;
    }
    const long acq_split = hostsim::counters.acq_split_launches.load() - acq_split0;
    std::printf("acquisition sweep: %ld calls launched, %ld rejected, %ld with G > 1 (%ld host statistics)\n", acq_launched, acq_rejected, acq_split, acq_stats_ok);
    EXPECT(acq_launched > calls / 16 && acq_rejected > calls / 64 && acq_split > calls / 64, "the acquisition sweep launched, rejected and split");

    // ---- 1d. the antenna-array entry points (gat_array_api.cpp) ------------------------------------------------------------
    {
        const auto &ct = hostsim::counters;
        auto cov_launches = [&]() { return ct.cov_small_launches.load() + ct.cov_tiled_launches.load() + ct.cov_finish_launches.load(); };
        long arr_ok = 0, arr_rejected = 0, arr_split = 0, arr_multi = 0, arr_stream = 0, arr_batched = 0;
        gat_ctx *shared = nullptr;
        EXPECT(gat_create(0, GAT_OWN_STREAM, &shared) == GAT_OK, "context for the array sweep");
        // one covariance call on real memory of exactly the signal's extent; returns the status
        auto cov_call = [&](gat_ctx *c, int fmt, int M, long long N, int B, int bpe, long long as, long long bs, size_t mis, int bad) {
            const size_t sb = (size_t)layout_sample_bytes(fmt);
            const size_t extent = ((size_t)(M - 1) * (size_t)as + (size_t)(B - 1) * (size_t)bs + (size_t)N) * sb;
            unsigned char *p_re = static_cast<unsigned char *>(std::malloc(extent + mis)), *p_im = fmt == 0 ? static_cast<unsigned char *>(std::malloc(extent + mis)) : nullptr;
            p_re[mis] = 1, p_re[mis + extent - 1] = 1;
            if (p_im) p_im[mis] = 1, p_im[mis + extent - 1] = 1;
            gat_signal_desc sig = {p_re + mis, p_im ? p_im + mis : nullptr, fmt, M, N, as, bs, 0};
            const int E = (B + bpe - 1) / bpe;
            const size_t outs = (size_t)E * M * M;
            float *c_re = static_cast<float *>(std::malloc(outs * sizeof(float))), *c_im = static_cast<float *>(std::malloc(outs * sizeof(float)));
            std::memset(c_re, 0xff, outs * sizeof(float));
            std::memset(c_im, 0xff, outs * sizeof(float));
            const gat_signal_desc *sigp = &sig;
            float *o_re = c_re, *o_im = c_im;
            gat_ctx *cc = c;
            int calls_B = B, calls_bpe = bpe;
            int32_t want = GAT_OK;
            switch (bad) { // one way to be wrong, or (0) none
            case 1: sigp = nullptr, want = GAT_ERR_ARG; break;
            case 2: o_re = nullptr, want = GAT_ERR_ARG; break;
            case 3: o_im = nullptr, want = GAT_ERR_ARG; break;
            case 4: cc = nullptr, want = GAT_ERR_ARG; break;
            case 5: calls_B = (int)uni(-2, 0), want = GAT_ERR_ARG; break;
            case 6: calls_bpe = (int)uni(-2, 0), want = GAT_ERR_ARG; break;
            case 7: sig.layout = (int)pick<long long>({-1, 4, 17}), want = GAT_ERR_ARG; break;
            case 8: sig.im = fmt == 0 ? nullptr : (void *)p_re, want = GAT_ERR_ARG; break; // planar without im, interleaved with one
            case 9: sig.num_ants = 65, want = GAT_ERR_RANGE; break;
            case 10: sig.chan_stride = pick<long long>({1, -1, as}), want = GAT_ERR_UNSUPPORTED; break;
            case 11: // zero (or negative) strides where the signal has several antennas or blocks
                if (M > 1 && (B == 1 || uni(0, 1))) sig.ant_stride = -uni(0, 1);
                else if (B > 1) sig.block_stride = -uni(0, 1);
                else sig.num_samples = 0;
                want = GAT_ERR_ARG;
                break;
            case 12: // an extent no double holds exactly
                if (B > 1) sig.block_stride = 9100000000000000ll;
                else if (M > 1) sig.ant_stride = 9100000000000000ll;
                else sig.num_samples = 9100000000000000ll;
                want = GAT_ERR_RANGE;
                break;
            case 13: sig.num_ants = (int)uni(-1, 0), want = GAT_ERR_ARG; break;
            case 14: sig.re = nullptr, want = GAT_ERR_ARG; break;
            default: break;
            }
            hostsim::cov_cover.reset(sig.re, B, N, bs);
            const long l0 = cov_launches(), small0 = ct.cov_small_launches, split0 = ct.cov_split_launches, multi0 = ct.cov_multi_unit_launches, fin0 = ct.cov_finish_launches;
            const long mallocs0 = ct.mallocs;
            const int32_t rc = gat_spatial_covariance(cc, sigp, calls_B, calls_bpe, o_re, o_im);
            EXPECT(rc == want, "covariance (case %d): status %d, want %d (%s): layout %d M %d N %lld B %d bpe %d strides %lld / %lld mis %zu", bad, rc, want,
                   c ? gat_last_error(c) : "", fmt, M, N, B, bpe, as, bs, mis);
            if (want != GAT_OK) {
                EXPECT(cov_launches() == l0 && ct.mallocs == mallocs0, "covariance (case %d): a refused call launched or allocated", bad);
                ++arr_rejected;
            } else if (rc == GAT_OK) {
                ++arr_ok;
                const bool vec = ct.cov_small_launches > small0;
                const long long vs = layout_vec_samples(fmt);
                const bool aligned = M <= gat::kCovSmallMaxAnts && mis % 16 == 0 && (M == 1 || as % vs == 0) && (B == 1 || bs % vs == 0);
                EXPECT(vec == aligned && (ct.cov_tiled_launches + ct.cov_small_launches - (l0 - fin0)) == ct.cov_finish_launches - fin0,
                       "covariance: streaming kernel %d for aligned %d (layout %d M %d strides %lld / %lld mis %zu)", (int)vec, (int)aligned, fmt, M, as, bs, mis);
                arr_stream += vec;
                arr_split += ct.cov_split_launches > split0;
                arr_multi += ct.cov_multi_unit_launches > multi0;
                arr_batched += ct.cov_finish_launches - fin0 > 1;
                const auto &seen = hostsim::cov_cover.seen;
                const size_t once = (size_t)std::count(seen.begin(), seen.end(), (unsigned char)1);
                EXPECT(once == seen.size(), "covariance: %zu of %zu (block, sample) pairs read exactly once: layout %d M %d N %lld B %d bpe %d CUs %d", once, seen.size(),
                       fmt, M, N, B, bpe, c->num_cus);
                bool whole = true;
                for (size_t i = 0; i < outs && whole; ++i) whole = c_re[i] == 0.0f && c_im[i] == 0.0f;
                EXPECT(whole, "covariance: the outputs are not written whole (E %d M %d)", E, M);
                EXPECT(gat_sync(c) == GAT_OK, "sync");
            }
            std::free(p_re);
            std::free(p_im);
            std::free(c_re);
            std::free(c_im);
            return rc;
        };
        for (int it = 0; it < calls; ++it) {
            // three calls of four on a new context: its scratch is then exactly what the call asked for, and ASan sees a slice
            // beyond it (a reused, larger scratch would hide that)
            gat_ctx *c = shared;
            if (it % 4) EXPECT(gat_create(0, GAT_OWN_STREAM, &c) == GAT_OK, "context for one array call");
            c->num_cus = (int)pick<long long>({64, 80, 104, 128, 228, 256, 256, 304, 512}); // the simulated device's size: only this sweep's contexts
            const int fmt = (int)uni(0, 3);
            const size_t sb = (size_t)layout_sample_bytes(fmt);
            const long long vs = layout_vec_samples(fmt);
            int M = (int)(uni(0, 1) ? uni(1, 8) : uni(1, 64));
            long long N = (long long)std::llround(std::exp(unif(0.0, std::log(300000.0))));
            int B = (int)std::llround(std::exp(unif(0.0, std::log(6000.0))));
            if (uni(0, 9) == 0) B = (int)uni(4100, 6000), N = uni(1, 40); // more blocks than any device wants workgroups
            if (uni(0, 9) == 0) B = (int)uni(1, 3), N = uni(20000, 300000); // long blocks: split
            while ((double)B * (double)N > 1.5e6 || (double)M * (double)B * (double)N * (double)sb > 24e6) { // bounded: table and signal
                if (B > 1 && uni(0, 1)) B = (B + 1) / 2;
                else if (N > 1) N = (N + 1) / 2;
                else M = (M + 1) / 2;
            }
            const int bpe = (int)pick<long long>({1, 1, uni(1, B), uni(1, B), B, B + uni(1, 5)});
            const bool tidy = uni(0, 2) != 0; // aligned base and strides of whole 16-byte loads: the streaming kernel where M <= 8
            const size_t mis = tidy ? 0 : (size_t)pick<long long>({0, 1, 1, 3}) * sb;
            long long bs = tidy ? (N + vs - 1) / vs * vs + vs * pick<long long>({0, 0, 1, 4}) : N + pick<long long>({0, 1, 3, 7});
            if (B == 1 && uni(0, 3) == 0) bs = 0;
            long long as = (B - 1) * bs + N;
            as = tidy ? (as + vs - 1) / vs * vs + vs * pick<long long>({0, 0, 2}) : as + pick<long long>({0, 1, 5});
            if (M == 1 && uni(0, 3) == 0) as = 0;
            const int bad = uni(0, 7) == 0 ? (int)uni(1, 14) : 0;
            cov_call(c, fmt, M, N, B, bpe, as, bs, mis, bad);
            if (c != shared) EXPECT(gat_destroy(c) == GAT_OK, "destroy");
        }
        // The estimate batch loop: M = 64, one block of N = 1 per estimate, E = 8192 + 5 > e_max = 256 MB / 32 KB: two launches, the
        // second with planes and outputs offset.  256 MB of scratch and 2 x 134 MB of outputs: fits comfortably here under ASan.
        {
            gat_ctx *c = nullptr;
            EXPECT(gat_create(0, GAT_OWN_STREAM, &c) == GAT_OK, "context for the batch loop");
            const long b0 = arr_batched;
            EXPECT(cov_call(c, GAT_LAYOUT_INTERLEAVED_I8, 64, 1, 8192 + 5, 1, 8192 + 5 + 3, 1, 0, 0) == GAT_OK && arr_batched == b0 + 1, "covariance: the estimate batch loop");
            EXPECT(gat_destroy(c) == GAT_OK, "destroy");
        }

        // weights, beamforming and the weighted update on real buffers of exactly the documented sizes
        long w_ok = 0, w_rej = 0, bf_ok = 0, bf_rej = 0, up_ok = 0, up_rej = 0, run_ok = 0, run_rej = 0, run_replayed = 0;
        const int n_other = std::max(40, calls / 8);
        for (int it = 0; it < n_other; ++it) {
            gat_ctx *c = shared;
            if (it % 2) EXPECT(gat_create(0, GAT_OWN_STREAM, &c) == GAT_OK, "context for one weights call");
            const int M = (int)pick<long long>({1, 2, 3, 5, 8, 9, 33, 63, 64, uni(1, 64)}), K = (int)pick<long long>({1, 1, 3, 64, 65, 1000, 65535, uni(1, 300)});
            const int mode = (int)uni(0, 2);
            std::vector<float> cre((size_t)M * M, 1.f), cim((size_t)M * M, 0.f);
            std::vector<double> sre((size_t)K * M, 1.0), sim((size_t)K * M, 0.0), wre((size_t)K * M, -1.0), wim((size_t)K * M, -1.0);
            const float *pcre = mode == GAT_BF_CONVENTIONAL && uni(0, 1) ? nullptr : cre.data(), *pcim = pcre ? cim.data() : nullptr;
            const double *psre = mode == GAT_BF_POWER_INVERSION && uni(0, 1) ? nullptr : sre.data(), *psim = psre ? sim.data() : nullptr;
            double *pwre = wre.data();
            int cM = M, cK = K, cmode = mode;
            double loading = pick<double>({0.0, 1e-3, 0.5});
            int32_t want = GAT_OK;
            switch (uni(0, 24)) {
            case 0: cmode = (int)pick<long long>({-1, 3, 9}), want = GAT_ERR_ARG; break;
            case 1: if (mode != GAT_BF_POWER_INVERSION) psim = nullptr, want = GAT_ERR_ARG; break;
            case 2: if (mode != GAT_BF_CONVENTIONAL) pcre = nullptr, want = GAT_ERR_ARG; break;
            case 3: loading = pick<double>({-1e-3, (double)NAN, (double)INFINITY}), want = GAT_ERR_ARG; break;
            case 4: pwre = nullptr, want = GAT_ERR_ARG; break;
            case 5: cK = (int)pick<long long>({0, -1}), want = GAT_ERR_ARG; break;
            case 6: cM = 65, want = GAT_ERR_RANGE; break;
            case 7: cK = 65536, want = GAT_ERR_RANGE; break;
            default: break;
            }
            const long l0 = ct.array_weight_launches;
            const int32_t rc = gat_array_weights(c, pcre, pcim, cM, psre, psim, cK, cmode, loading, pwre, wim.data());
            EXPECT(rc == want, "weights: status %d, want %d (%s): M %d K %d mode %d", rc, want, gat_last_error(c), cM, cK, cmode);
            if (want == GAT_OK && rc == GAT_OK) {
                EXPECT(ct.array_weight_launches == l0 + 1 && std::all_of(wre.begin(), wre.end(), [](double v) { return v == 0.0; }) &&
                           std::all_of(wim.begin(), wim.end(), [](double v) { return v == 0.0; }), "weights: launched once, the outputs written whole");
                ++w_ok;
            } else {
                EXPECT(ct.array_weight_launches == l0, "weights: a refused call launched");
                ++w_rej;
            }
            // beamform
            const int B = (int)pick<long long>({1, 2, 5, 64}), L = (int)pick<long long>({1, 3, 5, 32}), Kb = std::min(K, 300);
            const size_t rows = (size_t)B * Kb * L;
            std::vector<float> are(rows * M, 1.f), aim(rows * M, 1.f), yre(rows, -1.f), yim(rows, -1.f);
            int bB = B, bL = L;
            const float *pare = are.data();
            want = GAT_OK;
            switch (uni(0, 14)) {
            case 0: pare = nullptr, want = GAT_ERR_ARG; break;
            case 1: bB = 0, want = GAT_ERR_ARG; break;
            case 2: bL = -1, want = GAT_ERR_ARG; break;
            default: break;
            }
            const long bl0 = ct.beamform_launches;
            const int32_t rb = gat_beamform(c, pare, aim.data(), bB, Kb, bL, M, sre.data(), sim.data(), yre.data(), yim.data());
            EXPECT(rb == want, "beamform: status %d, want %d", rb, want);
            if (want == GAT_OK && rb == GAT_OK) {
                EXPECT(ct.beamform_launches == bl0 + 1 && std::all_of(yre.begin(), yre.end(), [](float v) { return v == 0.f; }) &&
                           std::all_of(yim.begin(), yim.end(), [](float v) { return v == 0.f; }), "beamform: launched once, the outputs written whole");
                ++bf_ok;
            } else {
                EXPECT(ct.beamform_launches == bl0, "beamform: a refused call launched");
                ++bf_rej;
            }
            // the weighted update: null weights are the unweighted launch
            gat_loop_config cfg = {1e-3, 18.0, 1.0, fc, 1575.42e6, 0.0, 1.0, lc, L, 0, L / 2, L - 1};
            std::vector<gat_loop_state> st((size_t)Kb);
            std::vector<gat_channel_params> cur((size_t)Kb, gat_channel_params{1, 0, fc, 1000.0, 10.0, 0.0}), nxt((size_t)Kb);
            std::vector<float> ure((size_t)Kb * L * M, 2.f), uim((size_t)Kb * L * M, 3.f);
            const double *uw_re = sre.data(), *uw_im = sim.data();
            int uK = Kb;
            want = GAT_OK;
            bool plain = false;
            switch (uni(0, 14)) {
            case 0: uw_im = nullptr, want = GAT_ERR_ARG; break;
            case 1: uw_re = nullptr, want = GAT_ERR_ARG; break;
            case 2: cfg.late_index = L, want = GAT_ERR_RANGE; break;
            case 3: uK = 0, want = GAT_ERR_ARG; break;
            case 4: uw_re = uw_im = nullptr, plain = true; break;
            default: break;
            }
            const long ul0 = ct.weighted_update_launches, ol0 = ct.other_launches;
            const int32_t ru = gat_tracking_update_weighted(c, ure.data(), uim.data(), uK, M, &cfg, st.data(), cur.data(), nxt.data(), uw_re, uw_im);
            EXPECT(ru == want, "weighted update: status %d, want %d (%s)", ru, want, gat_last_error(c));
            if (want == GAT_OK && ru == GAT_OK) {
                EXPECT(plain ? (ct.other_launches == ol0 + 1 && ct.weighted_update_launches == ul0) : ct.weighted_update_launches == ul0 + 1, "weighted update: the launch");
                ++up_ok;
            } else {
                EXPECT(ct.weighted_update_launches == ul0 && ct.other_launches == ol0, "weighted update: a refused call launched");
                ++up_rej;
            }
            EXPECT(gat_sync(c) == GAT_OK, "sync");
            if (c != shared) EXPECT(gat_destroy(c) == GAT_OK, "destroy");
        }
        // the weighted native run, eager and as a graph (the same arguments again: replayed), on the context that has the codes
        {
            const int K = 6, M = 4, L = 3, N = 20000, NB = 5;
            int32_t sh[3];
            EXPECT(gat_sample_shifts(L, N / 1e-3, fc, 0.5, sh) == GAT_OK, "sample shifts");
            gat_signal_desc sig = {(void *)0x10000000, (void *)0x50000000, GAT_LAYOUT_PLANAR, M, N, (long long)N * NB, N, 0};
            gat_loop_config cfg = {1e-3, 18.0, 1.0, fc, 1575.42e6, 0.0, 1.0, lc, L, 0, 1, 2};
            void *state, *pa, *pb, *are, *aim, *wre, *wim;
            gat_malloc(ctx, sizeof(gat_loop_state) * K, &state);
            gat_memset(ctx, state, 0, sizeof(gat_loop_state) * K);
            gat_malloc(ctx, sizeof(gat_channel_params) * K, &pa);
            gat_malloc(ctx, sizeof(gat_channel_params) * K, &pb);
            std::vector<gat_channel_params> p0(K, gat_channel_params{1, 0, fc, 1000.0, 10.0, 0.0});
            gat_memcpy_h2d(ctx, pa, p0.data(), sizeof(gat_channel_params) * K);
            gat_memcpy_h2d(ctx, pb, p0.data(), sizeof(gat_channel_params) * K);
            gat_malloc(ctx, sizeof(float) * NB * K * L * M, &are);
            gat_malloc(ctx, sizeof(float) * NB * K * L * M, &aim);
            gat_memset(ctx, are, 0, sizeof(float) * NB * K * L * M);
            gat_memset(ctx, aim, 0, sizeof(float) * NB * K * L * M);
            gat_malloc(ctx, sizeof(double) * K * M, &wre);
            gat_malloc(ctx, sizeof(double) * K * M, &wim);
            gat_memset(ctx, wre, 0, sizeof(double) * K * M);
            gat_memset(ctx, wim, 0, sizeof(double) * K * M);
            int32_t is_b = 0;
            const int reps = std::max(20, calls / 8);
            for (int rep = 0; rep < reps; ++rep) {
                const int nb = 1 + rep % 2 * (NB - 1); // (two block counts: their graphs stay in the LRU and are replayed)
                const uint32_t flags = rep % 3 == 0 ? 0u : GAT_FLAG_GRAPH;
                const bool bad = rep % 10 == 9, plain = rep % 10 == 4;
                const long ul0 = ct.weighted_update_launches, g0 = ct.graph_launches, gi0 = ct.graphs;
                const int32_t rr = gat_tracking_run_weighted(ctx, &sig, nb, K, L, sh, N / 1e-3, &cfg, (gat_loop_state *)state, (gat_channel_params *)pa,
                                                             (gat_channel_params *)pb, (float *)are, (float *)aim, (long long)K * L * M, flags, &is_b,
                                                             plain ? nullptr : (double *)wre, plain || bad ? nullptr : (double *)wim);
                if (bad) {
                    EXPECT(rr == GAT_ERR_ARG && ct.weighted_update_launches == ul0, "weighted run: one null weight plane returned %d", rr);
                    ++run_rej;
                    continue;
                }
                EXPECT(rr == GAT_OK && is_b == (nb & 1), "weighted run %d: %d (%s)", rep, rr, gat_last_error(ctx));
                const long ul = ct.weighted_update_launches - ul0;
                if (plain) EXPECT(ul == 0, "weighted run without weights launched %ld weighted updates", ul);
                else if (!flags) EXPECT(ul == nb, "weighted run: %ld weighted updates for %d blocks", ul, nb);
                else EXPECT((ul == 2 * nb && ct.graphs == gi0 + 1) || (ul == 0 && ct.graph_launches == g0 + 1), // recorded (one eager pass, one captured) or replayed
                            "weighted graph run: %ld updates, %ld replays", ul, ct.graph_launches - g0);
                run_replayed += !plain && flags && ul == 0;
                ++run_ok;
            }
            EXPECT(run_replayed >= 3, "the weighted run's graphs were replayed (%ld times)", run_replayed);
            EXPECT(gat_sync(ctx) == GAT_OK, "sync");
            for (void *p : {state, pa, pb, are, aim, wre, wim}) gat_free(ctx, p);
        }
        EXPECT(gat_destroy(shared) == GAT_OK, "destroy");
        std::printf("array sweep: %ld covariance calls launched, %ld rejected, %ld with splits > 1, %ld with more units than workgroups, %ld through the streaming kernel\n",
                    arr_ok, arr_rejected, arr_split, arr_multi, arr_stream);
        std::printf("array entry points: %ld / %ld weights, %ld / %ld beamform, %ld / %ld weighted updates, %ld / %ld weighted runs launched / rejected; %ld covariance calls in batches\n",
                    w_ok, w_rej, bf_ok, bf_rej, up_ok, up_rej, run_ok, run_rej, arr_batched);
        EXPECT(arr_ok > calls / 2 && arr_rejected > calls / 20 && arr_split > calls / 40 && arr_multi > calls / 40 && arr_stream > calls / 10 && arr_batched >= 1,
               "the array sweep launched, rejected, split, looped over units and batched");
    }

    // ---- 2. closed loop, stand-alone operators, groups ---------------------------------------------------------------------
    {
        const int K = 6, M = 4, L = 3, N = 20000, NB = 9;
        int32_t sh[3];
        EXPECT(gat_sample_shifts(L, N / 1e-3, fc, 0.5, sh) == GAT_OK && sh[0] < 0 && sh[1] == 0 && sh[2] > 0, "sample shifts");
        gat_signal_desc sig = {(void *)0x10000000, (void *)0x50000000, GAT_LAYOUT_PLANAR, M, N, (long long)N * NB, N, 0};
        gat_loop_config cfg = {1e-3, 18.0, 1.0, fc, 1575.42e6, 0.0, 1.0, lc, L, 0, 1, 2};
        void *state, *pa, *pb, *are, *aim;
        gat_malloc(ctx, sizeof(gat_loop_state) * K, &state);
        gat_memset(ctx, state, 0, sizeof(gat_loop_state) * K);
        gat_malloc(ctx, sizeof(gat_channel_params) * K, &pa);
        gat_malloc(ctx, sizeof(gat_channel_params) * K, &pb);
        std::vector<gat_channel_params> p0(K, gat_channel_params{1, 0, fc, 1000.0, 10.0, 0.0});
        gat_memcpy_h2d(ctx, pa, p0.data(), sizeof(gat_channel_params) * K);
        gat_malloc(ctx, sizeof(float) * NB * K * L * M, &are);
        gat_malloc(ctx, sizeof(float) * NB * K * L * M, &aim);
        int32_t is_b = 0;
        for (int rep = 0; rep < 7; ++rep) { // the same arguments again: graph replay; different block counts: the LRU
            const int nb = rep < 4 ? NB : NB - (rep - 3);
            EXPECT(gat_tracking_run(ctx, &sig, nb, K, L, sh, N / 1e-3, &cfg, (gat_loop_state *)state, (gat_channel_params *)pa, (gat_channel_params *)pb,
                                    (float *)are, (float *)aim, (long long)K * L * M, GAT_FLAG_GRAPH, &is_b) == GAT_OK, "tracking run %d: %s", rep, gat_last_error(ctx));
        }
        EXPECT(hostsim::counters.graph_launches >= 3, "the repeated tracking run replays its graph (%ld replays)", hostsim::counters.graph_launches.load());
        { // the loop's update on the host (needs no device): K channels of the accumulators left in `are` / `aim`
            std::vector<gat_loop_state> hs(K);
            std::vector<gat_channel_params> hc(K, gat_channel_params{1, 0, fc, 1000.0, 10.0, 0.0}), hn(K);
            std::vector<float> hre((size_t)K * L * M, 100.f), him((size_t)K * L * M, -3.f);
            EXPECT(gat_tracking_update_host(hre.data(), him.data(), K, M, &cfg, hs.data(), hc.data(), hn.data()) == GAT_OK && hn[0].code_freq_hz > 0.0, "host loop update");
            EXPECT(gat_tracking_update_host(hre.data(), him.data(), K, M, &cfg, hs.data(), hc.data(), hc.data()) == GAT_OK, "host loop update in place");
            gat_loop_config badc = cfg;
            badc.prompt_index = L;
            EXPECT(gat_tracking_update_host(hre.data(), him.data(), K, M, &badc, hs.data(), hc.data(), hn.data()) == GAT_ERR_RANGE, "host loop update: tap index");
        }
        EXPECT(gat_tracking_update(ctx, (float *)are, (float *)aim, K, M, &cfg, (gat_loop_state *)state, (gat_channel_params *)pa, (gat_channel_params *)pb) == GAT_OK, "tracking update");
        void *rep;
        gat_malloc(ctx, sizeof(float) * (N + 2) * 2, &rep);
        EXPECT(gat_gen_code_replica(ctx, (float *)rep, N + 2, 3, fc, N / 1e-3, 5.5, -1) == GAT_OK, "replica");
        EXPECT(gat_gen_code_replica(ctx, (float *)rep, N + 2, 99, fc, N / 1e-3, 5.5, -1) == GAT_ERR_RANGE, "replica: prn");
        EXPECT(gat_gen_code_replica_multi(ctx, (float *)rep, N + 2, N + 2, 2, (gat_channel_params *)pa, N / 1e-3, -1) == GAT_OK, "replica, two rows");
        EXPECT(gat_reduce_cplx_multi(ctx, (float *)are, (float *)aim, 1000, 6, (float *)are, (float *)aim) == GAT_OK, "reduction");
        float ms = -1.f;
        EXPECT(gat_timer_start(ctx) == GAT_OK && gat_timer_stop(ctx, &ms) == GAT_OK && ms >= 0.f, "timer");
        {
            const int laps = (int)uni(0, 40);
            float iv[64];
            int32_t got = -1;
            for (int i = 0; i < laps; ++i) EXPECT(gat_timer_lap(ctx) == GAT_OK, "lap");
            const int32_t cap = (int32_t)uni(0, 64);
            EXPECT(gat_timer_laps(ctx, iv, cap, &got) == GAT_OK && got == std::min(std::max(laps - 1, 0), (int)cap), "laps: %d intervals of %d laps (capacity %d)", got, laps, cap);
            for (int i = 0; i < got; ++i) EXPECT(iv[i] >= 0.f, "lap interval");
            EXPECT(gat_timer_laps(ctx, iv, 64, &got) == GAT_OK && got == 0, "laps are forgotten once read");
            float each[3] = {-1.f, -1.f, -1.f};
            EXPECT(gat_debug_read_stream(ctx, rep, sizeof(float) * (N + 2) * 2 / 16 * 16, (int32_t)uni(0, 15), 3, each) == GAT_OK && each[2] >= 0.f, "read stream");
            EXPECT(gat_debug_read_stream(ctx, rep, 24, 0, 1, each) == GAT_ERR_ARG && gat_debug_read_stream(ctx, rep, 64, 16, 1, each) == GAT_ERR_RANGE, "read stream: refusals");
            EXPECT(gat_gen_code_replica_texaddr(ctx, (float *)rep, N + 2, 3, fc, N / 1e-3, 5.5, -1, (int32_t)uni(0, 32), (int32_t)uni(-1, 24)) == GAT_OK, "texture addressing study");
            EXPECT(gat_gen_code_replica_texaddr(ctx, (float *)rep, N + 2, 3, fc, N / 1e-3, 5.5, -1, 33, 8) == GAT_ERR_RANGE, "texture addressing study: bits");
        }
        char name[64];
        int32_t ver = 0, cus = 0;
        EXPECT(gat_device_info(ctx, name, sizeof name, &ver, &cus) == GAT_OK && cus == 256, "device info");
        for (void *p : {state, pa, pb, are, aim, rep}) gat_free(ctx, p);
    }
    {
        gat_group *grp = nullptr;
        const int32_t devs[3] = {0, 1, 0};
        EXPECT(gat_group_create(3, devs, &grp) == GAT_OK, "group");
        EXPECT(gat_group_set_codes(grp, codes.data(), lc, 32) == GAT_OK, "group codes");
        const int K = 7, M = 4, L = 3, N = 4000, B = 2;
        int32_t sh[3] = {-2, 0, 2}, first, count, total = 0;
        for (int r = 0; r < 3; ++r) {
            EXPECT(gat_group_shard(grp, K, r, &first, &count) == GAT_OK && first == total, "shard %d", r);
            total += count;
        }
        EXPECT(total == K && gat_group_shard(grp, K, 3, &first, &count) != GAT_OK, "shards cover the channels");
        std::vector<void *> bufs(3), ore(3), oim(3);
        std::vector<gat_signal_desc> sigs(3);
        for (int r = 0; r < 3; ++r) {
            gat_ctx *m = nullptr;
            EXPECT(gat_group_ctx(grp, r, &m) == GAT_OK, "member");
            gat_malloc(m, sizeof(float) * N * B * M * 2, &bufs[r]);
            gat_malloc(m, sizeof(float) * B * 3 * L * M, &ore[r]);
            gat_malloc(m, sizeof(float) * B * 3 * L * M, &oim[r]);
            sigs[r] = {bufs[r], (float *)bufs[r] + (size_t)N * B * M, GAT_LAYOUT_PLANAR, M, N, (long long)N * B, N, 0};
        }
        EXPECT(gat_group_replicate(grp, 0, bufs.data(), sizeof(float) * N * B * M * 2) == GAT_OK, "replicate");
        std::vector<gat_channel_params> prm((size_t)B * K, gat_channel_params{2, 0, fc, 500.0, 1.0, 0.0});
        EXPECT(gat_group_correlate(grp, sigs.data(), prm.data(), B, K, L, sh, N / 1e-3, (float *const *)ore.data(), (float *const *)oim.data(), 0) == GAT_OK,
               "group correlate: %s", gat_group_last_error(grp));
        std::vector<float> hre((size_t)B * K * L * M), him(hre.size());
        EXPECT(gat_group_gather(grp, (float *const *)ore.data(), (float *const *)oim.data(), B, K, L, M, hre.data(), him.data()) == GAT_OK, "gather");
        EXPECT(gat_group_sync(grp) == GAT_OK, "group sync");
        for (int r = 0; r < 3; ++r) {
            gat_ctx *m = nullptr;
            gat_group_ctx(grp, r, &m);
            gat_free(m, bufs[r]); gat_free(m, ore[r]); gat_free(m, oim[r]);
        }
        EXPECT(gat_group_destroy(grp) == GAT_OK, "group destroy");
    }

    // ---- 3. the resident correlator against an emulated device -------------------------------------------------------------
    long res_calls = 0, res_opened = 0, res_refused = 0, res_capacity_refused = 0;
    long open_cus = 0; // workgroups of the correlators left open on ctx (the simulated device holds one resident workgroup per unit)
    gat_ctx *probe_ctx = nullptr; // a context without open correlators: tells how many workgroups a refused geometry has
    EXPECT(gat_create(0, GAT_OWN_STREAM, &probe_ctx) == GAT_OK && gat_set_codes(probe_ctx, codes.data(), lc, 32) == GAT_OK, "probe context");
    for (int it = 0; it < 60; ++it) {
        const int fmt = (int)uni(0, 3), M = (int)pick<long long>({1, 2, 3, 4, 8, 16}), K = (int)pick<long long>({1, 1, 2, 3, 4, 5, 9, 12, 16, 17}), L = (int)pick<long long>({1, 3, 5, 7, 8, 9});
        long long N = pick<long long>({2048, 2500, 4096, 16384, 20000, 65536, 262144, uni(100, 100000)});
        if (uni(0, 4) != 0) N -= N % layout_vec_samples(fmt);
        if (N < layout_vec_samples(fmt)) N = layout_vec_samples(fmt);
        std::vector<int32_t> sh(L);
        const int spread = (int)pick<long long>({1, 8, 300, 1000, 1500});
        for (int l = 0; l < L; ++l) sh[l] = (int32_t)uni(-spread, spread);
        const uintptr_t mis = pick<long long>({0, 0, 0, 0, 8});
        gat_signal_desc sig = {(void *)(uintptr_t)(0x10000000 + mis), fmt == 0 ? (void *)(uintptr_t)(0x50000000 + mis) : nullptr, fmt, M, N, N * 4, N, 0};
        gat_resident_config cfg = {sizeof cfg, (uint32_t)pick<long long>({150, 400, 100000}), (uint32_t)pick<long long>({5, 50, 2000}), (uint32_t)pick<long long>({0, 5, 17}),
                                   (uint32_t)pick<long long>({0, 1, 8, 200}), (uint32_t)pick<long long>({0, 1, 64}), (uint32_t)pick<long long>({0, 1, 2})};
        gat_resident *res = nullptr;
        const gat_resident_config *const cfgp = uni(0, 4) ? &cfg : nullptr;
        const int32_t rc = gat_resident_open(ctx, &sig, K, L, sh.data(), N / 1e-3, cfgp, &res);
        std::vector<int32_t> sorted(sh);
        std::sort(sorted.begin(), sorted.end());
        const bool servable = K <= 16 && L <= 8 && sorted.back() - sorted.front() <= 2048 && N % layout_vec_samples(fmt) == 0 && mis == 0;
        if (rc == GAT_ERR_UNSUPPORTED && servable) {
            // refused for want of room: the same geometry opens on a context without open correlators, and its workgroups
            // together with those left open here are more than the device's 256 units hold
            gat_resident *probe = nullptr;
            gat_resident_info pi{};
            const int32_t prc = gat_resident_open(probe_ctx, &sig, K, L, sh.data(), N / 1e-3, cfgp, &probe);
            EXPECT(prc == GAT_OK && gat_resident_info_get(probe, &pi, sizeof pi) == GAT_OK, "capacity refusal: the geometry itself is servable (%d, %s)", prc, gat_last_error(probe_ctx));
            EXPECT(open_cus + pi.workgroups > 256, "refused %d workgroups beside %ld left open: room for 256", pi.workgroups, open_cus);
            if (probe) EXPECT(gat_resident_close(probe) == GAT_OK, "close probe");
            ++res_capacity_refused;
            continue;
        }
        EXPECT((rc == GAT_OK) == servable, "resident open: rc %d for fmt %d M %d K %d L %d N %lld span %d mis %d (%s)", rc, fmt, M, K, L, N, sorted.back() - sorted.front(),
               (int)mis, gat_last_error(ctx));
        if (rc != GAT_OK) {
            EXPECT(rc == GAT_ERR_UNSUPPORTED && res == nullptr, "resident open: refusal code %d", rc);
            ++res_refused;
            continue;
        }
        ++res_opened;
        gat_resident_info info;
        EXPECT(gat_resident_info_get(res, &info, sizeof info) == GAT_OK && info.workgroups >= 1 && info.launches == 1, "resident info");
        // what the emulated workgroups post, summed by the rule of the kernel's grid decode
        const int MT = M % 4 == 0 ? 4 : M % 3 == 0 ? 3 : M % 2 == 0 ? 2 : 1, AG = M / MT, SP = info.splits, KG = K;
        std::vector<int32_t> order(L);
        for (int l = 0; l < L; ++l) order[l] = l;
        std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return sh[x] < sh[y]; });
        std::vector<float> want_re((size_t)K * L * M, 0.f), want_im(want_re.size(), 0.f);
        for (int sp = 0; sp < SP; ++sp)
            for (int ag = 0; ag < AG; ++ag)
                for (int kg = 0; kg < KG; ++kg) {
                    const unsigned slot = (unsigned)((ag * SP + sp) * KG + kg);
                    for (int o = 0; o < 2 * MT * L; ++o) {
                        const int ml = o >> 1, m = ag * MT + ml % MT, l = order[ml / MT];
                        ((o & 1) ? want_im : want_re)[((size_t)kg * L + l) * M + m] += hostsim::resident_value(slot, o);
                    }
                }
        EXPECT(info.workgroups == SP * AG * KG, "resident geometry: %d workgroups, %d splits x %d tiles x %d channels", info.workgroups, SP, AG, KG);
        std::vector<gat_channel_params> prm(K, gat_channel_params{4, 0, fc, 1234.0, 17.25, 0.125});
        std::vector<float> r_re(want_re.size()), r_im(want_re.size());
        const int n_calls = (int)pick<long long>({3, 40, 150});
        for (int cidx = 0; cidx < n_calls; ++cidx) {
            if (uni(0, 2) == 0) std::this_thread::sleep_for(std::chrono::microseconds(uni(0, 600)));
            const long long off = uni(0, 3) * N;
            if (uni(0, 30) == 0) { // calls the validation must refuse leave the correlator usable
                prm[0].prn = 77;
                EXPECT(gat_resident_correlate(res, prm.data(), off, r_re.data(), r_im.data()) == GAT_ERR_RANGE, "resident: bad prn");
                prm[0].prn = 4;
                EXPECT(gat_resident_correlate(res, prm.data(), 1, r_re.data(), r_im.data()) != GAT_OK || layout_vec_samples(fmt) == 1, "resident: misaligned offset");
            }
            std::fill(r_re.begin(), r_re.end(), -1.f);
            const int32_t rcc = gat_resident_correlate(res, prm.data(), off, r_re.data(), r_im.data());
            EXPECT(rcc == GAT_OK, "resident call %d: %d (%s)", cidx, rcc, gat_last_error(ctx));
            EXPECT(r_re == want_re && r_im == want_im, "resident call %d: results (first %g, want %g)", cidx, r_re[0], want_re[0]);
            ++res_calls;
            if (uni(0, 60) == 0) EXPECT(gat_resident_park(res) == GAT_OK, "park");
            if (uni(0, 90) == 0) { // scratch traffic on the context while a resident kernel is there
                void *p = nullptr;
                gat_malloc(ctx, 4096, &p);
                gat_free(ctx, p);
            }
        }
        int loop_calls = 0;
        if (it % 3 == 0) { // the host-closed loop from native code: {resident call, host update} per block
            gat_loop_config lc_cfg = {};
            lc_cfg.block_seconds = 1e-3; lc_cfg.pll_bandwidth_hz = 18.0; lc_cfg.dll_bandwidth_hz = 1.0; lc_cfg.code_freq_nominal_hz = 1.023e6;
            lc_cfg.carrier_center_hz = 1575.42e6; lc_cfg.early_late_spacing_chips = 1.0; lc_cfg.code_length = lc; lc_cfg.num_taps = L;
            lc_cfg.early_index = 0; lc_cfg.prompt_index = L / 2; lc_cfg.late_index = L - 1;
            std::vector<gat_loop_state> st((size_t)K);
            std::vector<gat_channel_params> lp(prm);
            const int nb = uni(1, 5);
            std::vector<float> a_re(want_re.size() * (size_t)nb, -1.f), a_im(a_re.size(), -1.f);
            const int32_t rl = gat_resident_tracking_run(res, nb, 0, N, &lc_cfg, st.data(), lp.data(), a_re.data(), a_im.data(), (int64_t)want_re.size());
            EXPECT(rl == GAT_OK, "resident tracking run: %d (%s)", rl, gat_last_error(ctx));
            for (int b = 0; b < nb && rl == GAT_OK; ++b)
                EXPECT(std::equal(want_re.begin(), want_re.end(), a_re.begin() + (size_t)b * want_re.size()) &&
                       std::equal(want_im.begin(), want_im.end(), a_im.begin() + (size_t)b * want_im.size()), "resident tracking run: block %d's accumulators", b);
            if (rl == GAT_OK) loop_calls = nb;
            lc_cfg.num_taps = L + 1;
            EXPECT(gat_resident_tracking_run(res, 1, 0, N, &lc_cfg, st.data(), lp.data(), a_re.data(), a_im.data(), 0) == GAT_ERR_ARG, "resident tracking run: tap count");
            res_calls += loop_calls;
        }
        EXPECT(gat_resident_info_get(res, &info, sizeof info) == GAT_OK && info.calls == (uint64_t)(n_calls + loop_calls), "resident: %llu calls counted", (unsigned long long)info.calls);
        if (it % 9 == 4) { // a new code table invalidates it
            EXPECT(gat_set_codes(ctx, codes.data(), lc, 32) == GAT_OK, "rebind");
            EXPECT(gat_resident_correlate(res, prm.data(), 0, r_re.data(), r_im.data()) == GAT_ERR_STATE, "stale correlator");
        }
        EXPECT(open_cus + info.workgroups <= 256, "resident open accepted %d workgroups beside %ld left open", info.workgroups, open_cus);
        if (it % 7 != 3) EXPECT(gat_resident_close(res) == GAT_OK, "close"); // (the others die with the context)
        else open_cus += info.workgroups;
    }
    { // room on the device: every workgroup of every open correlator has to be resident at once
        const long long N = 262144;
        const int32_t sh3[3] = {-10, 0, 10};
        gat_signal_desc sig = {(void *)(uintptr_t)0x10000000, (void *)(uintptr_t)0x50000000, 0, 4, N, N * 4, N, 0};
        gat_resident_config cfg = {sizeof cfg, 100000, 2000, 0, 200, 0, 0};
        gat_resident *a = nullptr, *b = nullptr;
        gat_resident_info ia{};
        EXPECT(gat_resident_open(probe_ctx, &sig, 1, 3, sh3, N / 1e-3, &cfg, &a) == GAT_OK && gat_resident_info_get(a, &ia, sizeof ia) == GAT_OK && ia.workgroups > 128,
               "a correlator of > 128 workgroups (%d)", ia.workgroups);
        EXPECT(gat_resident_open(probe_ctx, &sig, 1, 3, sh3, N / 1e-3, &cfg, &b) == GAT_ERR_UNSUPPORTED && b == nullptr, "a second one beside it must be refused");
        EXPECT(gat_resident_park_all(probe_ctx) == GAT_OK && gat_resident_info_get(a, &ia, sizeof ia) == GAT_OK && ia.running == 0, "park_all");
        EXPECT(gat_resident_close(a) == GAT_OK && gat_resident_open(probe_ctx, &sig, 1, 3, sh3, N / 1e-3, &cfg, &b) == GAT_OK, "room again once the first is closed");
        EXPECT(gat_destroy(probe_ctx) == GAT_OK, "destroy probe context (one correlator still open)");
    }
    std::printf("resident correlator: %ld opened, %ld refused as unsupported (+ %ld for want of room), %ld calls answered; the emulated kernel was started %ld times and served %ld rings\n",
                res_opened, res_refused, res_capacity_refused, res_calls, hostsim::counters.resident_starts.load(), hostsim::counters.resident_calls.load());
    EXPECT(res_opened > 10 && res_refused > 3 && hostsim::counters.resident_starts > res_opened, "the resident sweep restarted kernels");
    EXPECT(gat_destroy(ctx) == GAT_OK, "destroy");
    EXPECT(hostsim::counters.violations == 0, "%ld planner invariants broken", hostsim::counters.violations.load());
    std::printf("%s: %d failures, %ld broken invariants, device allocations %ld / frees %ld\n", failures || hostsim::counters.violations ? "FAILED" : "ok", failures,
                hostsim::counters.violations.load(), hostsim::counters.mallocs.load(), hostsim::counters.frees.load());
    return failures || hostsim::counters.violations ? 1 : 0;
}
