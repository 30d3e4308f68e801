// Stand-alone check of the direct acquisition search's pure plan (csrc/gat_acq_plan.h): the call check it shares with
// gat_acquire_fft and acq_plan.  Every documented refusal must return its code and a message with nothing written, and where two
// faults meet the entry point's order decides; a few thousand random accepted calls must keep the group count within its caps,
// deal every (antenna, block) unit to one group as the grid kernel walks them, cover every (Doppler, code) bin with one tile of the
// launcher's grid, carve disjoint aligned scratch regions inside the call's bytes, and bound every replica index a tile's window
// touches; and G and the bytes of a handful of shapes are pinned as literal numbers, taken from the inline rule this header
// replaced.  Built with -fsanitize=address,undefined by tests/test_acquisition_plan_host.py.  No memory behind the descriptors is
// ever touched: the plan reads addresses, not data.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_acq_plan.h"

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

constexpr int kTableLength = 1023, kTablePrns = 37; // the bound code table of every call here

gat_signal_desc desc(int layout, int M, long long N, long long as, long long bs)
{
    gat_signal_desc d{};
    d.re = reinterpret_cast<const void *>(uintptr_t(0x100000000000ull));
    d.im = layout == GAT_LAYOUT_PLANAR ? reinterpret_cast<const void *>(uintptr_t(0x300000000000ull)) : nullptr;
    d.layout = layout;
    d.num_ants = M;
    d.num_samples = N;
    d.ant_stride = as;
    d.block_stride = bs;
    d.chan_stride = 0;
    return d;
}

gat_acq_config config(int D, int J, int s, long long first_shift, int Lc)
{
    gat_acq_config c{};
    c.struct_size = sizeof(gat_acq_config);
    c.num_doppler_bins = D;
    c.num_code_bins = J;
    c.code_step_samples = s;
    c.if_hz = 1000.0;
    c.code_freq_hz = 1.023e6;
    c.doppler_first_hz = -500.0;
    c.doppler_step_hz = 250.0;
    c.first_shift = first_shift;
    c.code_length = Lc;
    return c;
}

template <class T>
T poisoned()
{
    T v;
    std::memset(static_cast<void *>(&v), 0x5a, sizeof v);
    return v;
}
template <class T>
bool untouched(const T &v)
{
    const T q = poisoned<T>();
    return std::memcmp(&v, &q, sizeof v) == 0;
}

struct Call {
    gat_signal_desc sig;
    int B, P;
    std::vector<int32_t> prns;
    double fs;
    gat_acq_config cfg;
    int cus;
    bool own;
};

// the two steps as the entry point takes them; the plan and the normalised configuration are written only by an accepted call
Refusal plan_call(const Call &c, const gat_acq_config *cfg_in, AcqPlan *plan, gat_acq_config *norm)
{
    const Refusal r = acq_check_call(cfg_in, c.B, c.prns.data(), c.P, c.fs, kTableLength, kTablePrns, norm);
    return r.code != GAT_OK ? r : acq_plan(&c.sig, c.B, c.P, c.fs, norm, c.cus, c.own, plan);
}

void expect_refusal(const Call &c, bool null_config, int code, const char *msg, const char *what)
{
    AcqPlan p = poisoned<AcqPlan>();
    gat_acq_config k = poisoned<gat_acq_config>();
    const Refusal r = plan_call(c, null_config ? nullptr : &c.cfg, &p, &k);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(r.msg != nullptr && std::strcmp(r.msg, msg) == 0, "%s: the message is %s", what, r.msg ? r.msg : "missing");
    CHECK(untouched(p), "%s: a refused call planned something", what);
    // the call check's refusals leave the normalised configuration alone too; acq_plan's come after it was written
    const bool by_check = !null_config && acq_check_call(&c.cfg, c.B, c.prns.data(), c.P, c.fs, kTableLength, kTablePrns, &k).code != GAT_OK;
    CHECK(!(null_config || by_check) || untouched(k), "%s: a refused call check wrote a configuration", what);
}

// every refusal, each from the valid call c, and the order where two faults meet
void refusals(const Call &c)
{
    const char *const empty = "empty grid (PRNs, Doppler bins and code bins must be positive)", *const chan = "chan_stride must be 0 (one signal for every PRN)";
    const char *const table = "config.code_length differs from the bound code table", *const blocks = "num_blocks must be positive";
    const char *const prn = "prn outside the code table", *const reach = "N + |first_shift| + s * J must stay below 2^30 samples";
    Call t = c;
    // the call check: the configuration (gat_acq_check.h), the table's length, the blocks, the PRNs
    expect_refusal(c, true, GAT_ERR_ARG, "null config", "null config");
    t = c, t.cfg.struct_size = 8;
    expect_refusal(t, false, GAT_ERR_ARG, "config.struct_size too small", "struct_size");
    t = c, t.cfg.reserved = 1;
    expect_refusal(t, false, GAT_ERR_ARG, "config.reserved must be 0", "reserved");
    t = c, t.P = 0;
    expect_refusal(t, false, GAT_ERR_ARG, empty, "no PRNs");
    t = c, t.cfg.num_doppler_bins = 0;
    expect_refusal(t, false, GAT_ERR_ARG, empty, "no Doppler bins");
    t = c, t.cfg.num_code_bins = -1;
    expect_refusal(t, false, GAT_ERR_ARG, empty, "no code bins");
    t = c, t.cfg.code_step_samples = 0;
    expect_refusal(t, false, GAT_ERR_ARG, "code step must be at least one sample", "no code step");
    t = c, t.cfg.code_step_samples = kAcqMaxCodeStep + 1;
    expect_refusal(t, false, GAT_ERR_RANGE, "code step above 31 samples", "code step 32");
    t = c, t.cfg.num_doppler_bins = 4096, t.cfg.num_code_bins = 20000;
    expect_refusal(t, false, GAT_ERR_RANGE, "grid above 2^26 bins", "above 2^26 bins");
    t = c, t.fs = 0.0;
    expect_refusal(t, false, GAT_ERR_ARG, "sampling frequency must be positive", "no sampling frequency");
    t = c, t.fs = INFINITY;
    expect_refusal(t, false, GAT_ERR_ARG, "sampling frequency must be positive", "infinite sampling frequency");
    t = c, t.cfg.code_freq_hz = -1.0;
    expect_refusal(t, false, GAT_ERR_ARG, "code frequency must be positive", "negative code frequency");
    t = c, t.cfg.if_hz = NAN;
    expect_refusal(t, false, GAT_ERR_ARG, "bad frequency / threshold", "NaN frequency");
    t = c, t.cfg.min_peak_ratio = -1.0;
    expect_refusal(t, false, GAT_ERR_ARG, "bad frequency / threshold", "negative threshold");
    t = c, t.cfg.if_hz = 3.0e12;
    expect_refusal(t, false, GAT_ERR_RANGE, "carrier frequency out of range", "carrier out of range");
    t = c, t.cfg.code_length = kTableLength + 1;
    expect_refusal(t, false, GAT_ERR_ARG, table, "another table's length");
    t = c, t.B = 0;
    expect_refusal(t, false, GAT_ERR_ARG, blocks, "no blocks");
    t = c, t.prns[(size_t)c.P - 1] = -1;
    expect_refusal(t, false, GAT_ERR_RANGE, prn, "negative PRN");
    t = c, t.prns[0] = kTablePrns;
    expect_refusal(t, false, GAT_ERR_RANGE, prn, "PRN past the table");
    // acq_plan: the descriptor, the reach, the code span, the grid's z axis
    t = c, t.sig.layout = 4;
    expect_refusal(t, false, GAT_ERR_ARG, "bad layout", "bad layout");
    t = c, t.sig.layout = -1;
    expect_refusal(t, false, GAT_ERR_ARG, "bad layout", "negative layout");
    t = c, t.sig.im = c.sig.layout == GAT_LAYOUT_PLANAR ? nullptr : t.sig.re;
    expect_refusal(t, false, GAT_ERR_ARG, "bad signal planes", "signal planes");
    t = c, t.sig.re = nullptr;
    expect_refusal(t, false, GAT_ERR_ARG, "bad signal planes", "no signal plane");
    t = c, t.sig.num_samples = 0;
    expect_refusal(t, false, GAT_ERR_ARG, "bad signal sizes", "no samples");
    t = c, t.sig.num_ants = 0;
    expect_refusal(t, false, GAT_ERR_ARG, "bad signal sizes", "no antennas");
    t = c, t.sig.ant_stride = -1;
    expect_refusal(t, false, GAT_ERR_ARG, "bad signal sizes", "negative ant_stride");
    t = c, t.sig.block_stride = -1;
    expect_refusal(t, false, GAT_ERR_ARG, "bad signal sizes", "negative block_stride");
    t = c, t.sig.chan_stride = 8;
    expect_refusal(t, false, GAT_ERR_ARG, chan, "chan_stride");
    if (c.sig.num_ants > 1) {
        t = c, t.sig.ant_stride = 0;
        expect_refusal(t, false, GAT_ERR_ARG, "ant_stride must be positive", "zero ant_stride");
        t = c, t.sig.ant_stride = 1ll << 60;
        expect_refusal(t, false, GAT_ERR_RANGE, "signal extent too large", "extent");
    }
    if (c.B > 1) {
        t = c, t.sig.block_stride = 0;
        expect_refusal(t, false, GAT_ERR_ARG, "block_stride must be positive", "zero block_stride");
    }
    t = c, t.cfg.first_shift = 1ll << 30;
    expect_refusal(t, false, GAT_ERR_RANGE, reach, "first_shift of 2^30 samples");
    t = c, t.cfg.first_shift = -(1ll << 30);
    expect_refusal(t, false, GAT_ERR_RANGE, reach, "first_shift of -2^30 samples");
    t = c, t.sig.num_samples = (1ll << 30) - kAcqChunk - std::llabs(c.cfg.first_shift) - (long long)c.cfg.code_step_samples * ((c.cfg.num_code_bins + 255) / 256) * 256;
    t.sig.block_stride = t.sig.num_samples, t.sig.ant_stride = t.sig.num_samples * c.B;
    expect_refusal(t, false, GAT_ERR_RANGE, reach, "the first N whose reach is 2^30"); // the tiles' unused code bins count
    // the order where two faults meet: configuration < table < blocks < PRNs < descriptor < reach < code span
    t = c, t.cfg.reserved = 1, t.cfg.code_length = kTableLength + 1, t.B = 0;
    expect_refusal(t, false, GAT_ERR_ARG, "config.reserved must be 0", "configuration ahead of the table and the blocks");
    t = c, t.cfg.code_step_samples = 40, t.prns[0] = -1;
    expect_refusal(t, false, GAT_ERR_RANGE, "code step above 31 samples", "configuration ahead of the PRNs");
    t = c, t.cfg.code_length = 5, t.B = 0, t.prns[0] = -1;
    expect_refusal(t, false, GAT_ERR_ARG, table, "table ahead of the blocks and the PRNs");
    t = c, t.B = -1, t.prns[0] = kTablePrns, t.sig.layout = 7;
    expect_refusal(t, false, GAT_ERR_ARG, blocks, "blocks ahead of the PRNs and the descriptor");
    t = c, t.prns[0] = kTablePrns, t.sig.num_ants = 0, t.cfg.first_shift = 1ll << 31;
    expect_refusal(t, false, GAT_ERR_RANGE, prn, "PRNs ahead of the descriptor and the reach");
    t = c, t.sig.chan_stride = 1, t.cfg.first_shift = 1ll << 31;
    expect_refusal(t, false, GAT_ERR_ARG, chan, "descriptor ahead of the reach");
    t = c, t.sig.layout = 9, t.sig.re = nullptr, t.sig.num_samples = 0;
    expect_refusal(t, false, GAT_ERR_ARG, "bad layout", "layout ahead of the planes and the sizes");
}

// what a call of a table other than kTableLength chips and of many PRNs is refused for
void table_refusals()
{
    // 2^21 laps of a three-chip code: inside the reach, beyond the code span
    const gat_signal_desc s = desc(GAT_LAYOUT_INTERLEAVED, 1, 1000, 1000, 1000);
    gat_acq_config k = config(3, 100, 1, 20000000, 3), norm = poisoned<gat_acq_config>();
    const int32_t prn = 0;
    AcqPlan p = poisoned<AcqPlan>();
    Refusal r = acq_check_call(&k, 1, &prn, 1, 2.0e6, 3, 1, &norm);
    CHECK(r.code == GAT_OK && norm.code_length == 3, "the three-chip call's check: %d", r.code);
    r = acq_plan(&s, 1, 1, 2.0e6, &norm, 256, true, &p);
    CHECK(r.code == GAT_ERR_RANGE && r.msg && !std::strcmp(r.msg, "code phase span too large") && untouched(p), "code phase span: %d %s", r.code, r.msg ? r.msg : "");
    k = config(3, 100, 1, 1ll << 31, 3);
    r = acq_check_call(&k, 1, &prn, 1, 2.0e6, 3, 1, &norm);
    if (r.code == GAT_OK) r = acq_plan(&s, 1, 1, 2.0e6, &norm, 256, true, &p);
    CHECK(r.code == GAT_ERR_RANGE && r.msg && std::strstr(r.msg, "2^30") && untouched(p), "the reach ahead of the code span: %d %s", r.code, r.msg ? r.msg : "");
    // more PRNs than the grid's z axis has workgroups: 65535 pass with one group, 65536 do not
    std::vector<int32_t> lots(65536, 5);
    k = config(1, 1, 1, 0, 0);
    for (int P : {65535, 65536}) {
        p = poisoned<AcqPlan>();
        r = acq_check_call(&k, 2, lots.data(), P, 2.0e6, kTableLength, kTablePrns, &norm);
        CHECK(r.code == GAT_OK && norm.code_length == kTableLength && norm.struct_size == sizeof(gat_acq_config), "%d PRNs: the call check: %d", P, r.code);
        r = acq_plan(&s, 2, P, 2.0e6, &norm, 256, true, &p);
        if (P == 65535)
            CHECK(r.code == GAT_OK && p.G == 1, "65535 PRNs: %d, G %d", r.code, p.G);
        else
            CHECK(r.code == GAT_ERR_RANGE && r.msg && !std::strcmp(r.msg, "too many PRNs for one call") && untouched(p), "65536 PRNs: %d %s", r.code, r.msg ? r.msg : "");
    }
}

// everything an accepted call promises
void check_plan(const Call &c, const gat_acq_config &k, const AcqPlan &p)
{
    const int M = c.sig.num_ants, B = c.B, P = c.P, D = k.num_doppler_bins, J = k.num_code_bins, s = k.code_step_samples;
    const long long N = c.sig.num_samples, units = (long long)M * B, cells = (long long)P * D * J;
    CHECK(p.cells == cells, "cells %lld of %lld", p.cells, cells);
    CHECK(p.G >= 1 && p.G <= units, "G %d of %lld units", p.G, units);
    CHECK((long long)P * p.G <= 65535, "%d PRNs x %d groups on the grid's z axis", P, p.G);
    CHECK(p.G == 1 || (double)p.G * (double)cells * 4.0 <= 1073741824.0, "%d slices of %lld cells", p.G, cells);
    const long long wgs = (long long)P * p.jtiles * p.dtiles;
    CHECK(wgs < 2ll * c.cus || p.G == 1, "%lld workgroups fill %d compute units, yet %d groups", wgs, c.cus, p.G);
    // the kernel's walk: workgroup z = p G + g takes the units g, g + G, ..., unit u = antenna u mod M of block u / M
    std::vector<unsigned char> unit_hits((size_t)units, 0);
    for (int g = 0; g < p.G; ++g) {
        long long mine = 0;
        for (long long u = g; u < units; u += p.G, ++mine) {
            const long long m = u % M, b = u / M;
            CHECK(u % p.G == g && m < M && b < B, "unit %lld of group %d: antenna %lld block %lld", u, g, m, b);
            if (b < B) ++unit_hits[(size_t)(b * M + m)];
        }
        CHECK(mine >= 1, "group %d has no unit", g);
    }
    for (size_t u = 0; u < unit_hits.size(); ++u)
        if (unit_hits[u] != 1) {
            CHECK(false, "unit %zu dealt %d times", u, (int)unit_hits[u]);
            break;
        }
    // the launcher's grid, and every (Doppler, code) bin in one tile: lane l of wave w owns Doppler bins d0 + 8 w .. + 7, code bins j0 + l + 64 r
    CHECK(p.jtiles == (J + kAcqCodeTile - 1) / kAcqCodeTile && p.dtiles == (D + kAcqDopTile - 1) / kAcqDopTile, "%d x %d tiles of a %d x %d grid", p.jtiles, p.dtiles, J, D);
    std::vector<unsigned char> bin_hits((size_t)D * (size_t)J, 0);
    long long x_lo = 0, x_hi = 0; // the replica indices the windows touch
    const long long last_n0 = (N - 1) / kAcqChunk * kAcqChunk, window = kAcqChunk + (long long)s * (kAcqCodeTile - 1);
    for (int tj = 0; tj < p.jtiles; ++tj) {
        const long long j0 = (long long)tj * kAcqCodeTile;
        const long long lo = k.first_shift + s * j0, hi = last_n0 + k.first_shift + s * j0 + window - 1; // chunks n0 = 0 .. last_n0, e < window
        x_lo = tj == 0 || lo < x_lo ? lo : x_lo, x_hi = tj == 0 || hi > x_hi ? hi : x_hi;
        for (int td = 0; td < p.dtiles; ++td)
            for (int i = td * kAcqDopTile; i < (td + 1) * kAcqDopTile && i < D; ++i)
                for (long long j = j0; j < j0 + kAcqCodeTile && j < J; ++j) ++bin_hits[(size_t)i * (size_t)J + (size_t)j];
    }
    for (size_t i = 0; i < bin_hits.size(); ++i)
        if (bin_hits[i] != 1) {
            CHECK(false, "bin (%zu, %zu) in %d tiles", i / (size_t)J, i % (size_t)J, (int)bin_hits[i]);
            break;
        }
    // the furthest index is within N rounded up to a chunk + |first_shift| + s jtiles 256, and that within the reach that was bounded
    const long long furthest = std::llabs(x_lo) > std::llabs(x_hi) ? std::llabs(x_lo) : std::llabs(x_hi);
    const long long bound = (N + kAcqChunk - 1) / kAcqChunk * kAcqChunk + std::llabs(k.first_shift) + (long long)s * p.jtiles * kAcqCodeTile;
    CHECK(furthest <= bound && (double)bound <= p.reach && p.reach < 1073741824.0, "windows reach %lld, bound %lld, planned reach %g", furthest, bound, p.reach);
    // the scratch: [256 bytes | results | power | slices | prns], disjoint, aligned for their elements, inside bytes
    const size_t res_bytes = (size_t)P * sizeof(gat_acq_result), pow_bytes = c.own ? (size_t)cells * 4 : 0, part_bytes = p.G > 1 ? (size_t)p.G * (size_t)cells * 4 : 0;
    CHECK(p.off_res == 256 && p.off_res % alignof(gat_acq_result) == 0 && p.off_res + res_bytes <= p.off_pow, "results at %zu, power at %zu", p.off_res, p.off_pow);
    CHECK(p.off_pow % 256 == 0 && p.off_pow + pow_bytes <= p.off_part, "power at %zu for %zu bytes, slices at %zu", p.off_pow, pow_bytes, p.off_part);
    CHECK(c.own || p.off_part == p.off_pow, "a power region of %zu bytes beside a caller's grid", p.off_part - p.off_pow);
    CHECK(p.off_part % 256 == 0 && p.off_part + part_bytes == p.off_prn, "slices at %zu for %zu bytes, prns at %zu", p.off_part, part_bytes, p.off_prn);
    CHECK(p.off_prn % alignof(int32_t) == 0 && p.off_prn + (size_t)P * 4 == p.bytes, "prns at %zu of %zu bytes", p.off_prn, p.bytes);
}

// the inline rule of gat_acquire that gat_acq_plan.h replaced, evaluated for these shapes before it went: G and the bytes of a call
// of 1000 samples.  The first three caps on G -- the units, two workgroups a compute unit, 1 GiB of slices -- and the grid's z axis
// each bind in one row at least; the last two cannot on a device of 304 compute units or fewer (the workgroups are at least
// cells / 8192 and P, so two a compute unit ask for less than 2^28 / cells and than 65535 / P groups): those rows plan for 2^20.
void pinned_numbers()
{
    const struct { int M, B, P, D, J; bool own; int cus; int G; size_t bytes; } rows[] = {
        {4, 1, 32, 29, 2000, true, 64, 1, 7426944ull},     // GPS L1, 32 PRNs: the grid alone fills 64 compute units
        {4, 1, 32, 29, 2000, true, 256, 2, 22274944ull},   // two workgroups a compute unit bind
        {4, 1, 32, 29, 2000, true, 304, 3, 29698944ull},
        {2, 3, 2, 5, 300, true, 64, 6, 84552ull},          // the units bind
        {2, 3, 2, 5, 300, true, 256, 6, 84552ull},
        {2, 3, 2, 5, 300, true, 304, 6, 84552ull},
        {2, 3, 2, 33, 300, false, 64, 6, 475720ull},       // a caller's grid: no power region
        {2, 3, 2, 33, 300, false, 304, 6, 475720ull},
        {16, 40, 1, 1, 1, true, 64, 128, 1284ull},         // one bin: 2 x 64, 2 x 256 groups, then the 640 units
        {16, 40, 1, 1, 1, true, 256, 512, 2820ull},
        {16, 40, 1, 1, 1, true, 304, 608, 3204ull},
        {16, 40, 1, 4096, 16384, true, 256, 1, 268435972ull}, // 2^26 bins: one group, its power grid the scratch
        {16, 40, 8, 640, 4096, false, 304, 1, 1056ull},
        {16, 40, 40000, 1, 1, true, 304, 1, 3520256ull},   // 65535 / P = 1
        {1, 1, 1, 1, 1, true, 64, 1, 772ull},
        {3, 5, 7, 31, 257, true, 64, 10, 2455044ull},
        {3, 5, 7, 31, 257, true, 256, 15, 3570424ull},
        {16, 40, 1, 4096, 16384, true, 1 << 20, 4, 1342177796ull}, // 1 GiB of slices binds: 4 of 2^26 cells
        {16, 40, 200, 1, 1, false, 1 << 20, 327, 278784ull},       // the grid's z axis binds: 65535 / 200
    };
    for (const auto &w : rows) {
        Call c{desc(GAT_LAYOUT_PLANAR, w.M, 1000, 100000, 1000), w.B, w.P, std::vector<int32_t>((size_t)w.P, 0), 4.0e6, config(w.D, w.J, 1, 0, kTableLength), w.cus, w.own};
        AcqPlan p = poisoned<AcqPlan>();
        gat_acq_config k;
        const Refusal r = plan_call(c, &c.cfg, &p, &k);
        CHECK(r.code == GAT_OK && p.G == w.G && p.bytes == w.bytes, "pinned: M %d B %d P %d D %d J %d on %d CUs: %d, G %d (%d), %zu bytes (%zu)", w.M, w.B, w.P, w.D, w.J, w.cus,
              r.code, p.G, w.G, p.bytes, w.bytes);
    }
    std::printf("pinned %zu plans\n", sizeof rows / sizeof rows[0]);
}

} // namespace

int main()
{
    std::mt19937_64 rng(20261020);
    auto pick = [&](long long lo, long long hi) { return (long long)(rng() % (uint64_t)(hi - lo + 1)) + lo; };
    pinned_numbers();
    table_refusals();
    int planned = 0, grouped = 0, own_grid = 0, refused_from = 0;
    int layouts[4] = {};
    for (int it = 0; it < 4500; ++it) {
        const int layout = (int)pick(0, 3), M = (int)pick(1, 16), B = (int)pick(1, 40), P = (int)pick(1, 40), s = (int)pick(1, kAcqMaxCodeStep);
        const int D = (int)(it % 3 == 0 ? pick(1, 100) : pick(1, 33)), J = (int)(it % 4 == 0 ? pick(1, 3000) : pick(1, 600));
        const long long N = it % 5 == 0 ? pick(1, 300) : pick(1, 30000), first_shift = it % 7 == 0 ? 0 : pick(-5000, 5000);
        const long long bs = N + pick(0, 9), as = bs * B + pick(0, 5);
        Call c{desc(layout, M, N, as, bs), B, P, std::vector<int32_t>((size_t)P), 2.0e6, config(D, J, s, first_shift, it % 2 ? kTableLength : 0), (int)pick(1, 304), it % 3 != 1};
        for (auto &v : c.prns) v = (int32_t)pick(0, kTablePrns - 1);
        AcqPlan p = poisoned<AcqPlan>();
        gat_acq_config k = poisoned<gat_acq_config>();
        const Refusal r = plan_call(c, &c.cfg, &p, &k);
        CHECK(r.code == GAT_OK && r.msg == nullptr, "a valid call was refused: %d %s", r.code, r.msg ? r.msg : "");
        if (r.code != GAT_OK) continue;
        ++planned, grouped += p.G > 1, own_grid += c.own, ++layouts[layout];
        // the normalised configuration: the caller's, with its size and the table's length filled in
        gat_acq_config want = c.cfg;
        want.struct_size = sizeof(gat_acq_config), want.code_length = kTableLength;
        CHECK(std::memcmp(&k, &want, sizeof k) == 0, "the normalised configuration differs from the caller's");
        check_plan(c, k, p);
        if (it % 9 == 0) refusals(c), ++refused_from;
    }
    CHECK(planned >= 4000 && grouped > planned / 5 && planned - grouped > planned / 10 && own_grid > planned / 2 && layouts[0] > 800 && layouts[1] > 800 && layouts[2] > 800 && layouts[3] > 800,
          "the sweep lost its balance: %d planned, %d with groups, %d with the plan's grid", planned, grouped, own_grid);
    std::printf("planned %d calls (%d with unit groups, %d with a caller's grid), every refusal from %d of them, %d failures\n", planned, grouped, planned - own_grid, refused_from,
                failures);
    return failures ? 1 : 0;
}
