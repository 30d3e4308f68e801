// Stand-alone check of the two rules that host and kernels must agree on bit for bit: which channel record a kernel can evaluate
// exactly (csrc/gat_chan_rules.h: the kernels' predicates and the host's refusals, which are their negation) and how a code table
// lies in device memory (csrc/gat_code_tables.h: strides, refusals, packers).  Every refusal of the host checks with its code and
// message; over random draws of (record, N, max shift, Lc, fs, P) a record the host accepts is never one a kernel poisons; a record
// that breaks one rule alone is refused on the host and bad on the device; the bounds one ulp either side; and the packed tables of
// every length from 1 to 130 chips, 1023, 10230 and 120000, in exactly sized buffers.  Built with -fsanitize=address,undefined and
// -ffp-contract=off (the span is a multiply followed by adds) by tests/test_channel_rules_host.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "gat_chan_rules.h"
#include "gat_code_tables.h"

using namespace gat;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                      \
    do {                                                      \
        if (!(cond)) {                                        \
            if (++failures <= 20) {                           \
                std::printf("FAIL %s:%d: ", #cond, __LINE__); \
                std::printf(__VA_ARGS__);                     \
                std::printf("\n");                            \
            }                                                 \
        }                                                     \
    } while (0)

std::mt19937_64 rng(20261020ull);
long long uni(long long lo, long long hi) { return std::uniform_int_distribution<long long>(lo, hi)(rng); }
double unif(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(rng); }
template <class T> T pick(std::initializer_list<T> l) { return *(l.begin() + uni(0, (long long)l.size() - 1)); }

constexpr double kInf = std::numeric_limits<double>::infinity(), kNaN = std::numeric_limits<double>::quiet_NaN();
double below(double x) { return std::nextafter(x, -kInf); }
double above(double x) { return std::nextafter(x, kInf); }

// ---- what the kernels evaluate (gat_kernels.hip, gat_dc_body.inc; the matrix kernels add mfma_wrap_bad, which the plan answers) ----
bool dev_correlator_bad(const gat_channel_params &p, int P, int Lc, double reach, double fs)
{
    return p.prn < 0 || p.prn >= P || code_span_bad(p.code_freq_hz / fs, p.code_phase_chips, reach, Lc) || carrier_bad(p.carrier_freq_hz / fs, p.carrier_phase_cycles);
}
// code_replica_multi_kernel's, for the one record of the one-channel generators
bool dev_replica_bad(int prn, int P, int Lc, double fc, double fs, double tau, long long count, long long first_shift)
{
    const double reach = (double)count + (double)(first_shift < 0 ? -first_shift : first_shift);
    return prn < 0 || prn >= P || code_span_bad(fc / fs, tau, reach, Lc);
}
// accumulate_debug_kernel's (the host hands it the PRN's row)
bool dev_accumulate_bad(const gat_channel_params &p, int Lc, long long N, long long max_shift, double fs)
{
    return code_span_bad(p.code_freq_hz / fs, p.code_phase_chips, (double)N + (double)max_shift, Lc);
}

bool is(const Refusal &r, int code, const char *msg) { return r.code == code && (msg ? r.msg && std::strcmp(r.msg, msg) == 0 : !r.msg); }
long refusals_seen = 0;
void expect_refusal(const Refusal &r, int code, const char *msg, int line)
{
    ++refusals_seen;
    CHECK(is(r, code, msg), "line %d: wanted %d (%s), got %d (%s)", line, code, msg, r.code, r.msg ? r.msg : "none");
}
#define EXPECT_REFUSAL(r, code, msg) expect_refusal((r), (code), (msg), __LINE__)

// a GPS L1 channel at 20 MHz: one block of 20000 samples, taps within 10 samples, 32 rows of 1023 chips
constexpr int kP = 32, kLc = 1023;
constexpr double kFs = 20.0e6, kReach = 20010.0;
const gat_channel_params kOk = {3, 0, 1.023e6, 1000.0, 0.5, 0.25};

// ---- every refusal of the three host checks and of the table check, with its code and message as literals ---------------------------
void refusals()
{
    const char *const prn = "prn outside the code table", *const span = "code phase span too large";
    auto records = [](const gat_channel_params &p) { return check_channel_records(&p, 1, kP, kLc, kReach, kFs); };
    CHECK(is(records(kOk), GAT_OK, nullptr), "the valid record");
    CHECK(is(check_channel_records(nullptr, 0, kP, kLc, kReach, kFs), GAT_OK, nullptr), "no record");
    gat_channel_params t = kOk;
    t.prn = -1, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, prn);
    t = kOk, t.prn = kP, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, prn);
    t = kOk, t.code_freq_hz = kNaN, EXPECT_REFUSAL(records(t), GAT_ERR_ARG, "non-finite channel parameter");
    t = kOk, t.carrier_freq_hz = kInf, EXPECT_REFUSAL(records(t), GAT_ERR_ARG, "non-finite channel parameter");
    t = kOk, t.code_phase_chips = -kInf, EXPECT_REFUSAL(records(t), GAT_ERR_ARG, "non-finite channel parameter");
    t = kOk, t.carrier_phase_cycles = kNaN, EXPECT_REFUSAL(records(t), GAT_ERR_ARG, "non-finite channel parameter");
    t = kOk, t.code_freq_hz = -1.0, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, "negative code frequency");
    t = kOk, t.carrier_freq_hz = 1.0e15 * kFs, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, "carrier frequency / phase out of range");
    t = kOk, t.carrier_phase_cycles = -1.0e15, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, "carrier frequency / phase out of range");
    t = kOk, t.code_phase_chips = 1073741824.0, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, span);
    // (the order: the first broken rule of the first bad record speaks)
    t = kOk, t.prn = kP, t.code_freq_hz = kNaN, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, prn);
    t = kOk, t.code_freq_hz = -1.0, t.carrier_phase_cycles = 2.0e15, t.code_phase_chips = 2.0e9, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, "negative code frequency");
    t = kOk, t.carrier_phase_cycles = 2.0e15, t.code_phase_chips = 2.0e9, EXPECT_REFUSAL(records(t), GAT_ERR_RANGE, "carrier frequency / phase out of range");
    {
        gat_channel_params two[2] = {kOk, kOk};
        two[1].prn = -1, two[0].code_phase_chips = 2.0e9;
        EXPECT_REFUSAL(check_channel_records(two, 2, kP, kLc, kReach, kFs), GAT_ERR_RANGE, span);
        two[0] = kOk;
        EXPECT_REFUSAL(check_channel_records(two, 2, kP, kLc, kReach, kFs), GAT_ERR_RANGE, prn);
        CHECK(is(check_channel_records(two, 1, kP, kLc, kReach, kFs), GAT_OK, nullptr), "the first of two records");
    }

    // the replica generators
    auto replica = [](long long count, int p, double fc, double fs, double tau, long long shift, bool exact) {
        return check_replica_call(count, p, kP, kLc, fc, fs, tau, shift, exact);
    };
    CHECK(is(replica(20000, 3, 1.023e6, kFs, 0.5, -10, true), GAT_OK, nullptr), "the valid replica");
    EXPECT_REFUSAL(replica(0, 3, 1.023e6, kFs, 0.5, 0, true), GAT_ERR_ARG, "count must be positive");
    EXPECT_REFUSAL(replica(20000, -1, 1.023e6, kFs, 0.5, 0, true), GAT_ERR_RANGE, prn);
    EXPECT_REFUSAL(replica(20000, kP, 1.023e6, kFs, 0.5, 0, false), GAT_ERR_RANGE, prn);
    EXPECT_REFUSAL(replica(20000, 3, 1.023e6, 0.0, 0.5, 0, true), GAT_ERR_ARG, "bad frequency / phase");
    EXPECT_REFUSAL(replica(20000, 3, 1.023e6, kNaN, 0.5, 0, true), GAT_ERR_ARG, "bad frequency / phase");
    EXPECT_REFUSAL(replica(20000, 3, kInf, kFs, 0.5, 0, true), GAT_ERR_ARG, "bad frequency / phase");
    EXPECT_REFUSAL(replica(20000, 3, 1.023e6, kFs, kNaN, 0, false), GAT_ERR_ARG, "bad frequency / phase");
    EXPECT_REFUSAL(replica(1ll << 30, 3, 1.023e6, kFs, 0.5, 0, true), GAT_ERR_RANGE, "replica too long");
    EXPECT_REFUSAL(replica(20000, 3, 1.023e6, kFs, 0.5, -((1ll << 30) - 20000), false), GAT_ERR_RANGE, "replica too long");
    EXPECT_REFUSAL(replica(20000, 3, 1.023e6, kFs, -2.0e9, 0, true), GAT_ERR_RANGE, span);
    EXPECT_REFUSAL(replica(20000, 3, -1.023e6, kFs, 0.5, 0, true), GAT_ERR_RANGE, span);
    // (the generators that clamp their coordinates instead take any finite span)
    CHECK(is(replica(20000, 3, 1.023e6, kFs, -2.0e9, 0, false), GAT_OK, nullptr), "a clamping generator far out");
    CHECK(is(replica(20000, 3, -1.023e6, kFs, 0.5, 0, false), GAT_OK, nullptr), "a clamping generator running backwards");

    // the accumulate call's one record
    auto accumulate = [](const gat_channel_params &p, long long N, long long ms, double fs) { return check_accumulate_record(p, kP, kLc, N, ms, fs); };
    CHECK(is(accumulate(kOk, 20000, 10, kFs), GAT_OK, nullptr), "the valid accumulate record");
    t = kOk, t.prn = -1, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_RANGE, prn);
    t = kOk, t.prn = kP, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_RANGE, prn);
    EXPECT_REFUSAL(accumulate(kOk, 20000, 10, 0.0), GAT_ERR_ARG, "bad frequency / phase");
    EXPECT_REFUSAL(accumulate(kOk, 20000, 10, kNaN), GAT_ERR_ARG, "bad frequency / phase");
    t = kOk, t.code_freq_hz = kInf, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_ARG, "bad frequency / phase");
    t = kOk, t.code_freq_hz = -1.0, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_ARG, "bad frequency / phase");
    t = kOk, t.code_freq_hz = kNaN, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_ARG, "bad frequency / phase");
    t = kOk, t.carrier_freq_hz = kNaN, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_ARG, "bad frequency / phase");
    t = kOk, t.code_phase_chips = kInf, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_ARG, "bad frequency / phase");
    t = kOk, t.carrier_phase_cycles = -kInf, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_ARG, "bad frequency / phase");
    EXPECT_REFUSAL(accumulate(kOk, 20000, (1ll << 30) - 20000, kFs), GAT_ERR_RANGE, "num_samples + |shift| must stay below 2^30");
    t = kOk, t.code_phase_chips = 2.0e9, EXPECT_REFUSAL(accumulate(t, 20000, 10, kFs), GAT_ERR_RANGE, span);

    // the table
    CHECK(is(check_code_table(1, 1), GAT_OK, nullptr) && is(check_code_table(120000, 1 << 20), GAT_OK, nullptr), "the smallest and the longest table");
    EXPECT_REFUSAL(check_code_table(0, 1), GAT_ERR_ARG, "sizes must be positive");
    EXPECT_REFUSAL(check_code_table(1023, 0), GAT_ERR_ARG, "sizes must be positive");
    EXPECT_REFUSAL(check_code_table(-5, -5), GAT_ERR_ARG, "sizes must be positive");
    EXPECT_REFUSAL(check_code_table(120001, 1), GAT_ERR_RANGE, "code table does not fit in LDS (max 120000 chips)");
}

// ---- a record that breaks one rule alone: refused by the host with that rule's message, bad on the device -----------------------------
void single_rules()
{
    struct One {
        const char *rule;
        gat_channel_params p;
        int Lc;
        int code;
        const char *msg;
    };
    auto with = [](auto set) { gat_channel_params p = kOk; set(p); return p; };
    const One rules[] = {
        {"prn below the table", with([](auto &p) { p.prn = -1; }), kLc, GAT_ERR_RANGE, "prn outside the code table"},
        {"prn beyond the table", with([](auto &p) { p.prn = kP; }), kLc, GAT_ERR_RANGE, "prn outside the code table"},
        {"code frequency NaN", with([](auto &p) { p.code_freq_hz = kNaN; }), kLc, GAT_ERR_ARG, "non-finite channel parameter"},
        {"code frequency inf", with([](auto &p) { p.code_freq_hz = kInf; }), kLc, GAT_ERR_ARG, "non-finite channel parameter"},
        {"carrier frequency inf", with([](auto &p) { p.carrier_freq_hz = -kInf; }), kLc, GAT_ERR_ARG, "non-finite channel parameter"},
        {"code phase NaN", with([](auto &p) { p.code_phase_chips = kNaN; }), kLc, GAT_ERR_ARG, "non-finite channel parameter"},
        {"carrier phase inf", with([](auto &p) { p.carrier_phase_cycles = kInf; }), kLc, GAT_ERR_ARG, "non-finite channel parameter"},
        {"code frequency negative", with([](auto &p) { p.code_freq_hz = -1.023e6; }), kLc, GAT_ERR_RANGE, "negative code frequency"},
        {"carrier step of 10^15 cycles", with([](auto &p) { p.carrier_freq_hz = -1.0e15 * kFs; }), kLc, GAT_ERR_RANGE, "carrier frequency / phase out of range"},
        {"carrier phase of 10^15 cycles", with([](auto &p) { p.carrier_phase_cycles = 1.0e15; }), kLc, GAT_ERR_RANGE, "carrier frequency / phase out of range"},
        {"span of 2^30 chips", with([](auto &p) { p.code_phase_chips = -1073741824.0; }), kLc, GAT_ERR_RANGE, "code phase span too large"},
        {"span of 2^21 laps", with([](auto &p) { p.code_phase_chips = 2097152.0 * 3.0; }), 3, GAT_ERR_RANGE, "code phase span too large"},
        {"span by the code rate", with([](auto &p) { p.code_freq_hz = 1.1e12; }), kLc, GAT_ERR_RANGE, "code phase span too large"},
    };
    for (const One &r : rules) {
        const Refusal got = check_channel_records(&r.p, 1, kP, r.Lc, kReach, kFs);
        CHECK(is(got, r.code, r.msg), "%s: host says %d (%s)", r.rule, got.code, got.msg ? got.msg : "none");
        CHECK(dev_correlator_bad(r.p, kP, r.Lc, kReach, kFs), "%s: not bad on the device", r.rule);
        // the same record with the rule kept passes both (the rule alone was broken)
        CHECK(is(check_channel_records(&kOk, 1, kP, r.Lc, kReach, kFs), GAT_OK, nullptr) && !dev_correlator_bad(kOk, kP, r.Lc, kReach, kFs), "%s: the record without it", r.rule);
    }
    // the matrix kernels' own rule is the plan's to keep (tests/corrplan): a record may break it alone and pass the host
    gat_channel_params fast = kOk;
    fast.code_freq_hz = kFs * 40.0;
    CHECK(mfma_wrap_bad(fast.code_freq_hz / kFs, kLc) && !mfma_wrap_bad(kOk.code_freq_hz / kFs, kLc), "the wrap rule on 40 and 0.05 chips a sample");
    CHECK(is(check_channel_records(&fast, 1, kP, kLc, kReach, kFs), GAT_OK, nullptr) && !dev_correlator_bad(fast, kP, kLc, kReach, kFs), "40 chips a sample on the vector kernel");
}

// ---- the bounds, one step either side ------------------------------------------------------------------------------------------------
void boundaries()
{
    // host and device on one record of a still code (ratio 0: span = |tau| + 1, exact) and fs = 1 (step = carrier frequency)
    auto both = [](const gat_channel_params &p, int Lc, bool want_ok, const char *what) {
        const bool host_ok = check_channel_records(&p, 1, kP, Lc, 1000.0, 1.0).code == GAT_OK, dev_ok = !dev_correlator_bad(p, kP, Lc, 1000.0, 1.0);
        CHECK(host_ok == want_ok && dev_ok == want_ok, "%s: host %s, device %s", what, host_ok ? "accepts" : "refuses", dev_ok ? "evaluates" : "poisons");
    };
    gat_channel_params t = {0, 0, 0.0, 0.0, 0.0, 0.0};
    // span = 2^30 - ulp, 2^30, 2^30 + ulp (tables of 512 chips and more: 2^21 Lc is no tighter)
    const double two30 = 1073741824.0;
    t.code_phase_chips = below(two30) - 1.0, both(t, 1023, true, "span one ulp below 2^30");
    CHECK(t.code_phase_chips + 1.0 == below(two30), "the span below 2^30 is exact");
    t.code_phase_chips = -(two30 - 1.0), both(t, 1023, false, "span 2^30");
    t.code_phase_chips = above(two30) - 1.0, both(t, 1023, false, "span one ulp above 2^30");
    CHECK(t.code_phase_chips + 1.0 == above(two30), "the span above 2^30 is exact");
    t.code_phase_chips = below(two30) - 1.0, both(t, 512, true, "span one ulp below 2^30 = 2^21 * 512");
    t.code_phase_chips = below(two30) - 1.0, both(t, 511, false, "span one ulp below 2^30 on 511 chips");
    // span either side of 2^21 Lc
    for (int Lc : {1, 3, 100}) {
        const double bound = 2097152.0 * Lc;
        t.code_phase_chips = below(bound) - 1.0, both(t, Lc, true, "span one ulp below 2^21 Lc");
        CHECK(t.code_phase_chips + 1.0 == below(bound), "the span below 2^21 Lc is exact");
        t.code_phase_chips = bound - 1.0, both(t, Lc, false, "span 2^21 Lc");
        t.code_phase_chips = -(above(bound) - 1.0), both(t, Lc, false, "span one ulp above 2^21 Lc");
    }
    // the span's multiply and adds, each rounded: 0.3 * 1000 + |0.1| + 1 as the device computes it
    CHECK(!code_span_bad(0.3, 0.1, 1000.0, 1023) && code_span_bad(0.3, 0.1, 1000.0, 0), "a table of no chips takes no record");
    t.code_phase_chips = 0.5;
    // the code rate: -0, NaN, +-inf (fs = 1: the ratio is the code frequency)
    t.code_freq_hz = -0.0, both(t, 1023, true, "ratio -0.0");
    CHECK(!code_span_bad(-0.0, 0.5, 1000.0, 1023) && code_span_bad(-4.9e-324, 0.5, 1000.0, 1023), "ratio -0.0 and the smallest negative ratio");
    t.code_freq_hz = kNaN, both(t, 1023, false, "ratio NaN");
    t.code_freq_hz = kInf, both(t, 1023, false, "ratio +inf");
    t.code_freq_hz = -kInf, both(t, 1023, false, "ratio -inf");
    CHECK(code_span_bad(kNaN, 0.5, 1000.0, 1023) && code_span_bad(kInf, 0.5, 1000.0, 1023) && code_span_bad(-kInf, 0.5, 1000.0, 1023) && code_span_bad(0.5, kNaN, 1000.0, 1023),
          "non-finite ratio and phase on the device");
    t.code_freq_hz = 0.5;
    // the carrier: 10^15 and its predecessor, both signs, step and phase
    for (double sign : {1.0, -1.0}) {
        t.carrier_freq_hz = sign * below(1.0e15), both(t, 1023, true, "carrier step below 10^15");
        t.carrier_freq_hz = sign * 1.0e15, both(t, 1023, false, "carrier step 10^15");
        t.carrier_freq_hz = 0.0;
        t.carrier_phase_cycles = sign * below(1.0e15), both(t, 1023, true, "carrier phase below 10^15");
        t.carrier_phase_cycles = sign * 1.0e15, both(t, 1023, false, "carrier phase 10^15");
        t.carrier_phase_cycles = 0.0;
    }
    CHECK(carrier_bad(kNaN, 0.0) && carrier_bad(0.0, kNaN) && carrier_bad(kInf, 0.0) && carrier_bad(0.0, -kInf) && !carrier_bad(0.0, 0.0), "non-finite carrier on the device");
    // the table's rows
    t.prn = -1, both(t, 1023, false, "prn -1");
    t.prn = kP, both(t, 1023, false, "prn P");
    t.prn = kP - 1, both(t, 1023, true, "prn P - 1");
    t.prn = 0;
    // one chip
    both(t, 1, true, "a table of one chip");
    // the matrix kernels' rule at its edge: 32 samples span the table exactly
    CHECK(!mfma_wrap_bad(below(1023.0 / 32.0), 1023) && mfma_wrap_bad(1023.0 / 32.0, 1023) && mfma_wrap_bad(kNaN, 1023) && !mfma_wrap_bad(-0.0, 1), "the wrap rule's edge");
}

// ---- accept implies not poisoned, over random draws ---------------------------------------------------------------------------------------
double draw_value(double typical)
{
    switch (uni(0, 15)) {
    case 0: return kNaN;
    case 1: return pick<double>({kInf, -kInf});
    case 2: return -typical * unif(0.0, 2.0);
    case 3: return pick<double>({0.0, -0.0});
    case 4: return pick<double>({1.0e15, -1.0e15, below(1.0e15), 1073741824.0, below(1073741824.0) - 1.0, 2097152.0, 1.0e9, -1.0e9, 1.0e300, -1.0e300});
    case 5: return typical * std::exp(unif(0.0, 40.0));
    default: return typical * unif(0.0, 2.0);
    }
}
long accepted[3], refused[3], draws = 0;
void sweep(long n)
{
    for (long it = 0; it < n; ++it, ++draws) {
        const int Lc = (int)pick<long long>({1, 2, 3, 64, 511, 512, 1023, 10230, 120000, uni(1, 120000)});
        const int P = (int)uni(1, 64);
        const double fs = uni(0, 9) ? unif(1.0e3, 1.0e8) : pick<double>({0.0, -0.0, -2.0e6, kNaN, kInf, -kInf, 4.9e-324, 1.0e-300, 1.0e300});
        const long long N = pick<long long>({1, uni(1, 5000), uni(1, 300000), uni(1, (1ll << 30) - 1)});
        const long long ms = pick<long long>({0, uni(0, 100), uni(0, 5000), uni(0, (1ll << 30) - 1)});
        gat_channel_params p;
        p.prn = uni(0, 7) ? (int32_t)uni(0, P - 1) : (int32_t)pick<long long>({-1, P, P + 5, INT32_MIN, INT32_MAX});
        p.reserved = 0;
        p.code_freq_hz = uni(0, 3) ? unif(0.0, 2.0) * 1.023e6 * pick<double>({1.0, 10.0}) : draw_value(1.023e6);
        p.carrier_freq_hz = uni(0, 3) ? unif(-1.0, 1.0) * 1.0e7 : draw_value(1.0e6);
        p.code_phase_chips = uni(0, 3) ? unif(-2.0, 2.0) * Lc : draw_value((double)Lc);
        p.carrier_phase_cycles = uni(0, 3) ? unif(-1.0, 1.0) : draw_value(1.0e3);
        const bool fs_ok = fs > 0.0 && std::isfinite(fs);

        // the correlator's records: accepted -> not poisoned, whatever fs; with the fs that the entry points let through, refused -> poisoned too
        const double reach = (double)(N + ms);
        const bool ok0 = check_channel_records(&p, 1, P, Lc, reach, fs).code == GAT_OK, bad0 = dev_correlator_bad(p, P, Lc, reach, fs);
        CHECK(!(ok0 && bad0), "draw %ld: the host accepts a record the correlator kernels poison (prn %d of %d, fc %g, f %g, tau %g, phi %g; Lc %d, fs %g, reach %g)", it, p.prn, P,
              p.code_freq_hz, p.carrier_freq_hz, p.code_phase_chips, p.carrier_phase_cycles, Lc, fs, reach);
        // (a negative code frequency below fs's smallest quotient is -0 chips a sample on the device: refused on the host all the same)
        if (fs_ok && !(p.code_freq_hz < 0.0 && p.code_freq_hz / fs == 0.0))
            CHECK(ok0 == !bad0, "draw %ld: the host refuses a record the correlator kernels evaluate (prn %d of %d, fc %g, f %g, tau %g, phi %g; Lc %d, fs %g, reach %g)", it, p.prn, P,
                  p.code_freq_hz, p.carrier_freq_hz, p.code_phase_chips, p.carrier_phase_cycles, Lc, fs, reach);
        ++(ok0 ? accepted : refused)[0];

        // the exact replica generator (its count and shift are the call's N and largest shift, either sign)
        const long long shift = uni(0, 1) ? ms : -ms;
        const bool ok1 = check_replica_call(N, p.prn, P, Lc, p.code_freq_hz, fs, p.code_phase_chips, shift, true).code == GAT_OK;
        CHECK(!(ok1 && dev_replica_bad(p.prn, P, Lc, p.code_freq_hz, fs, p.code_phase_chips, N, shift)), "draw %ld: the host accepts a replica the kernel poisons (fc %g, tau %g; Lc %d, fs %g, %lld + %lld)",
              it, p.code_freq_hz, p.code_phase_chips, Lc, fs, N, shift);
        ++(ok1 ? accepted : refused)[1];

        // the accumulate call's record
        const bool ok2 = check_accumulate_record(p, P, Lc, N, ms, fs).code == GAT_OK;
        CHECK(!(ok2 && dev_accumulate_bad(p, Lc, N, ms, fs)), "draw %ld: the host accepts a record the accumulate kernel poisons (fc %g, tau %g; Lc %d, fs %g, %lld + %lld)", it,
              p.code_freq_hz, p.code_phase_chips, Lc, fs, N, ms);
        CHECK(!ok2 || (fs > 0.0 && N + ms < (1ll << 30)), "draw %ld: the accumulate check let fs %g, %lld + %lld through", it, fs, N, ms); // (an infinite fs is a still code)
        ++(ok2 ? accepted : refused)[2];
    }
}

// ---- the packed tables ---------------------------------------------------------------------------------------------------------------------
// A caller's chip table as the host simulator draws it (tests/hostsim/main.cpp chip_table), P rows of Lc chips.  kind 0: random +-1;
// 1: +-1 with some chips 0; 2: {-1, 0, +1}; 3: the whole int8 range, -128 and 127 included.
std::vector<int8_t> chip_table(int Lc, int P, int kind)
{
    std::vector<int8_t> t((size_t)Lc * P);
    for (auto &v : t) v = kind == 3 ? (int8_t)uni(-128, 127) : kind == 2 ? (int8_t)uni(-1, 1) : (int8_t)(uni(0, 1) ? 1 : -1);
    if (kind == 1)
        for (int i = 0; i < std::max(1, Lc / 50); ++i) t[(size_t)uni(0, (long long)t.size() - 1)] = 0;
    return t;
}
long tables_packed = 0, bit_tables_packed = 0;
void pack_one(int Lc, int P, int kind)
{
    const std::vector<int8_t> t = chip_table(Lc, P, kind);
    const int rs = code_row_stride(Lc), bs = code_bits_stride(Lc);
    CHECK(rs % 16 == 0 && rs > Lc && rs <= Lc + 16, "%d chips: row stride %d", Lc, rs);
    CHECK(bs % 4 == 0 && (Lc >> 5) + 1 < bs && (bs - 4) * 32 < Lc + 1 + 32, "%d chips: bit stride %d", Lc, bs);
    // exactly sized storage, filled with what a packer must not leave behind
    std::unique_ptr<int8_t[]> rows(new int8_t[(size_t)rs * P]);
    std::memset(rows.get(), 0x5a, (size_t)rs * P);
    pack_code_rows(t.data(), Lc, P, rows.get());
    long wrong = 0;
    for (int p = 0; p < P; ++p) {
        const int8_t *row = rows.get() + (size_t)p * rs, *src = t.data() + (size_t)p * Lc;
        for (int i = 0; i < rs; ++i) wrong += row[i] != (i < Lc ? src[i] : i == Lc ? src[0] : 0);
    }
    CHECK(wrong == 0, "%d chips x %d, kind %d: %ld bytes of the rows differ (chips, the first chip again at Lc, zero padding)", Lc, P, kind, wrong);
    ++tables_packed;

    bool pm1 = true; // the test's own reading of "every chip is +-1"
    for (int8_t v : t) pm1 = pm1 && (v == 1 || v == -1);
    CHECK(codes_all_pm1(t.data(), Lc, P) == pm1 && (kind != 0 || pm1) && (kind != 1 || !pm1), "%d chips x %d, kind %d: +-1 test says %d", Lc, P, kind, (int)!pm1);
    if (!pm1) return; // bit tables are built for +-1 tables only
    std::unique_ptr<uint32_t[]> bits(new uint32_t[(size_t)bs * P]);
    std::memset(bits.get(), 0x5a, (size_t)bs * P * sizeof(uint32_t));
    pack_code_bits(t.data(), Lc, P, bits.get());
    wrong = 0;
    for (int p = 0; p < P; ++p) {
        const uint32_t *row = bits.get() + (size_t)p * bs;
        const int8_t *src = t.data() + (size_t)p * Lc;
        for (int i = 0; i < bs * 32; ++i) {
            const bool want = i < Lc ? src[i] < 0 : i == Lc ? src[0] < 0 : false; // bit Lc repeats bit 0, every other bit behind is zero
            wrong += ((row[i >> 5] >> (i & 31)) & 1u) != (want ? 1u : 0u);
        }
    }
    CHECK(wrong == 0, "%d chips x %d: %ld bits of the sign rows differ", Lc, P, wrong);
    ++bit_tables_packed;
}
void packers()
{
    for (int Lc = 1; Lc <= 130; ++Lc)
        for (int kind = 0; kind < 4; ++kind) pack_one(Lc, (int)uni(1, 4), kind);
    for (int Lc : {1023, 10230, 120000})
        for (int kind = 0; kind < 4; ++kind) pack_one(Lc, Lc == 120000 ? 2 : 3, kind);
    // a table of one row of one negative chip: both of its bits, nothing else
    const int8_t one = -1;
    uint32_t word[4] = {~0u, ~0u, ~0u, ~0u};
    pack_code_bits(&one, 1, 1, word);
    CHECK(word[0] == 3u && word[1] == 0u && word[2] == 0u && word[3] == 0u, "one negative chip: %08x", word[0]);
}

// Stride pairs as literals, worked out from the expressions gat_set_codes held: bytes (Lc + 16) & ~15, dwords (((Lc + 1 + 32 + 31) / 32) + 3) & ~3
constexpr int kPinnedStrides[][3] = {{1, 16, 4},     {15, 16, 4},     {16, 32, 4},      {31, 32, 4},        {32, 48, 4},        {63, 64, 4},           {64, 80, 4},
                                     {65, 80, 4},    {96, 112, 8},    {191, 192, 8},    {192, 208, 8},      {193, 208, 8},      {224, 240, 12},     {1023, 1024, 36},      {1024, 1040, 36},
                                     {10230, 10240, 324}, {20000, 20016, 628}, {119999, 120000, 3752}, {120000, 120016, 3752}};
static_assert(code_row_stride(1023) == 1024 && code_bits_stride(1023) == 36 && code_row_stride(10230) == 10240 && code_bits_stride(10230) == 324, "the L1 and L5 tables");
static_assert(kMaxCodeLength == 120000, "the longest table");
void pinned()
{
    for (const auto &r : kPinnedStrides)
        CHECK(code_row_stride(r[0]) == r[1] && code_bits_stride(r[0]) == r[2], "%d chips: strides %d bytes, %d dwords (pinned %d, %d)", r[0], code_row_stride(r[0]), code_bits_stride(r[0]), r[1], r[2]);
}

} // namespace

int main()
{
    refusals();
    single_rules();
    boundaries();
    sweep(120000);
    packers();
    pinned();
    for (int k = 0; k < 3; ++k) CHECK(accepted[k] > draws / 20 && refused[k] > draws / 20, "check %d: %ld accepted, %ld refused of %ld draws", k, accepted[k], refused[k], draws);
    std::printf("records: %ld accepted, %ld refused; replicas: %ld, %ld; accumulate records: %ld, %ld\n", accepted[0], refused[0], accepted[1], refused[1], accepted[2], refused[2]);
    std::printf("packed %ld tables (%ld with sign-bit rows), pinned %zu stride pairs\n", tables_packed, bit_tables_packed, sizeof(kPinnedStrides) / sizeof(kPinnedStrides[0]));
    std::printf("drew %ld calls, %ld refusals provoked, %d failures\n", draws, refusals_seen, failures);
    return failures ? 1 : 0;
}
