// Stand-alone check of the correlator call's pure plan (csrc/gat_corr_plan.h): corr_check_call, corr_plan and corr_plan_resident.
// A few thousand random calls -- every layout, aligned and off by one sample, ragged lengths, 1 .. 64 antennas and channels, 1 .. 32
// taps within and beyond one launch's span, L1- / L5-length and 20 000-chip tables with and without sign-bit rows, host and device
// records, both flag values, every knob drawn from its option range, devices of 8 .. 304 CUs -- must plan launches that keep what the
// kernels assume (tests/corr_launch_contract.h, shared with the host simulator's stand-in launchers) and that own every tap of the
// call exactly once, with the caller's index; every refusal that a call can reach must come with its code and message; every branch
// of the plan listed in `Branch` must be reached; inline host records that break the matrix kernels' wrap rule (mfma_wrap_bad) must keep a
// call away from them, and only those; and the geometry of the benchmark's shapes at 256 CUs is pinned as literal
// numbers, taken from the planner this header replaced.  Built with -fsanitize=address,undefined by
// tests/test_correlator_plan_host.py.  No memory behind the descriptors is ever touched: the plan reads addresses, not data.
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../corr_launch_contract.h"
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

// the launch contract's failure callback
__attribute__((format(printf, 2, 3))) void broken(const char *cond, const char *fmt, ...)
{
    if (++failures > 20) return;
    std::printf("FAIL launch contract: %s -- ", cond);
    va_list ap;
    va_start(ap, fmt);
    std::vprintf(fmt, ap);
    va_end(ap);
    std::printf("\n");
}

std::mt19937_64 rng(20261020ull);
long long uni(long long lo, long long hi) { return std::uniform_int_distribution<long long>(lo, hi)(rng); }
template <class T> T pick(std::initializer_list<T> l) { return *(l.begin() + uni(0, (long long)l.size() - 1)); }

// addresses the plan only looks at
template <class T> T *addr(uintptr_t a) { return reinterpret_cast<T *>(a); }
constexpr uintptr_t kRe = 0x100000000000ull, kIm = 0x300000000000ull;

// A bound code table as gat_set_codes leaves it (gat_code_tables.h): chip rows, and sign-bit rows where every chip is +-1
CorrTables tables(int Lc, bool bits, int cus)
{
    return {addr<const int8_t>(0x500000000000ull), bits ? addr<const uint32_t>(0x600000000000ull) : nullptr, addr<const void>(0x700000000000ull), Lc, 32,
            code_row_stride(Lc), bits ? code_bits_stride(Lc) : 0, cus};
}

// One call with everything it points to
struct Case {
    gat_signal_desc sig;
    int B, K, L;
    std::vector<int32_t> shifts;
    double fs;
    bool host; // host records (inside the arguments up to kInlineParams of them, uploaded beyond)
    std::vector<gat_channel_params> recs;
    uint32_t flags;
    CorrKnobs knobs;
    CorrTables tab;
    CorrCall call() const
    {
        const bool inl = host && (long long)B * K <= kInlineParams;
        return {&sig, inl ? nullptr : addr<const gat_channel_params>(0x800000000000ull), inl ? recs.data() : nullptr, B, K, L, shifts.data(), fs,
                addr<float>(0x900000000000ull), addr<float>(0xa00000000000ull), flags};
    }
};

gat_signal_desc desc(int fmt, int M, long long N, long long as, long long bs, long long cs = 0, uintptr_t off = 0)
{
    return {addr<void>(kRe + off), fmt == GAT_LAYOUT_PLANAR ? addr<void>(kIm + off) : nullptr, fmt, M, N, as, bs, cs};
}

// a shape as the benchmark builds it: contiguous [M][B][N] samples, taps (l - L / 2) * s, device records unless host
Case bench_case(int fmt, int Lc, double fc, long long N, int M, int L, int K, int B, int mc_mode, bool host, double block_s = 1e-3)
{
    Case c{desc(fmt, M, N, N * B, N), B, K, L, {}, (double)N / block_s, host, {}, 0u, CorrKnobs{}, tables(Lc, true, 256)};
    const int s = std::max(1, (int)std::lround(0.5 * c.fs / fc));
    for (int l = 0; l < L; ++l) c.shifts.push_back((l - L / 2) * s);
    c.recs.assign((size_t)std::min<long long>((long long)B * K, kInlineParams), gat_channel_params{0, 0, fc, 1000.0, 0.0, 0.0});
    c.knobs.mc_mode = mc_mode;
    return c;
}

Case random_case()
{
    Case c{};
    const int fmt = (int)uni(0, 3), vs = layout_vec_samples(fmt);
    const int M = (int)pick<long long>({1, 2, 3, 4, 4, 8, 12, 16, 16, 32, 48, 64, uni(1, 64)});
    c.K = (int)pick<long long>({1, 1, 2, 3, 4, 8, 12, 16, 32, 64, uni(1, 64)});
    c.B = M * c.K >= 256 ? (int)pick<long long>({1, 1, 2, 3}) : (int)pick<long long>({1, 1, 1, 2, 3, 7, 16, 64, 500, 4096});
    c.L = (int)pick<long long>({1, 2, 3, 3, 5, 7, 8, 11, 16, 17, 32, uni(1, 32)});
    long long N = pick<long long>({uni(1, 64), uni(64, 5000), 2048, 2500, 4096, 20000, 50000, uni(5000, 300000)});
    if (uni(0, 2) != 0) N -= N % vs; // otherwise ragged
    if (N < 1) N = vs;
    const long long bs = N + pick<long long>({0, 0, 0, 0, 0, vs, 32, 1, 3}), as = bs * c.B + pick<long long>({0, 0, 0, vs * 4, 1});
    const long long cs = c.K > 1 && uni(0, 5) == 0 ? as * M : 0;
    // the base: on a 128-byte line, on a 16-byte boundary off it, or off by one sample
    c.sig = desc(fmt, M, N, as, bs, cs, (uintptr_t)pick<long long>({0, 0, 0, 16, 64, layout_sample_bytes(fmt)}));
    const int spread = (int)pick<long long>({1, 2, 10, 128, 400, 700, 1024, 1500, 5000});
    for (int l = 0; l < c.L; ++l) c.shifts.push_back((int32_t)uni(-spread, spread));
    if (uni(0, 1)) std::sort(c.shifts.begin(), c.shifts.end());
    c.fs = (double)N / 1e-3;
    const int tbl = (int)uni(0, 2), Lc = tbl == 0 ? 1023 : tbl == 1 ? 10230 : 20000;
    c.tab = tables(Lc, uni(0, 1) != 0, (int)pick<long long>({8, 64, 104, 256, 304}));
    c.host = uni(0, 1) != 0;
    c.recs.assign((size_t)std::min<long long>((long long)c.B * c.K, kInlineParams), gat_channel_params{(int32_t)uni(0, 31), 0, tbl == 1 ? 10.23e6 : 1.023e6, 1000.0, 0.5, 0.25});
    // (now and then one host record beyond the matrix kernels' wrap rule, at its edge or past it: check_plan)
    if (c.host && uni(0, 7) == 0) c.recs[(size_t)uni(0, (long long)c.recs.size() - 1)].code_freq_hz = c.fs * Lc / 32.0 * pick<double>({1.0, 1.5});
    c.flags = uni(0, 5) == 0 ? GAT_FLAG_ATOMIC : 0u;
    // every knob: its default, or any value of its range (kOptions of gat_api.cpp; gat_set_matrix_core)
    CorrKnobs &k = c.knobs;
    auto draw = [](auto &member, long long lo, long long hi, std::initializer_list<long long> likely = {}) {
        if (uni(0, 3) != 0) return;
        member = (std::decay_t<decltype(member)>)(likely.size() && uni(0, 1) ? pick(likely) : uni(lo, hi));
    };
    if (uni(0, 1)) k.mc_mode = (int)uni(GAT_MC_VECTOR, GAT_MC_BF16_SPLIT); // (the kernel selection more often: few shapes suit a matrix kernel)
    draw(k.mc_nct, 0, 4);
    if (k.mc_nct == 3) k.mc_nct = 2; // (as the option stores it)
    draw(k.mc_i16_terms, 2, 3);
    draw(k.max_ant_tile, 1, kMaxAntTile);
    draw(k.max_aw, 1, 4);
    draw(k.max_kt, 1, 4);
    draw(k.max_bpw, 1, 1 << 20, {1, 2, 4, 64});
    draw(k.force_bpw, 0, 1 << 20, {0, 1, 3, 8});
    draw(k.wgs_per_cu, 0, 1024, {0, 1, 2, 16});
    draw(k.one_wave, 0, 1);
    draw(k.one_wave_min, -1, 1ll << 40, {-1, 0, 64});
    draw(k.one_wave_seg, 1, kUcarSteps);
    draw(k.max_depth, 1, 2);
    draw(k.keep_l2, -1, 1);
    draw(k.quads, -1, 1);
    draw(k.bit_tables, 0, 2);
    draw(k.aw2, -1, 1);
    draw(k.seg_cap, 0, kUcarSteps);
    draw(k.align_head, 0, 1);
    return c;
}

// The branches of the plan that the sweep must reach, counted per accepted call
enum Branch { kKind0, kKind1, kKind2, kOneWave, kTile2x2, kAw4Kt2, kAw4Kt4, kDepth2, kTail, kScalar, kTapGroups, kReplicaCopy, kAlignHead,
              kBitTables, kTwoTerm, kSplitFinalize, kBlocksPerWg, kBranches };
const char *const kBranchName[kBranches] = {"kind 0", "kind 1", "kind 2", "nw == 1", "the 2 x 2 tile", "aw 4 kt 2", "aw 4 kt 4", "depth 2", "a tail", "vec == 1",
                                            "several tap groups", "the shifted replica copy", "align_head", "sign-bit tables in the vector kernel",
                                            "the two-term int16 mode", "a split with finalize", "bpw > 1"};
long reached[kBranches];
long matrix_records_checked = 0; // inline host records of calls that a matrix kernel took

void count_branches(const CorrPlan &p)
{
    ++reached[p.kind == 0 ? kKind0 : p.kind == 1 ? kKind1 : kKind2];
    reached[kSplitFinalize] += p.splits > 1 && p.finalize;
    if (p.kind) {
        reached[kTwoTerm] += p.kind == 2 && p.m.mb_mode == kMbTwo;
        return;
    }
    const DcArgs &a = p.a[0];
    const DcLaunch &g = p.cfg[0];
    reached[kOneWave] += g.nw == 1;
    reached[kTile2x2] += g.aw == 2 && g.ant_tile == 2 && g.kt == 2;
    reached[kAw4Kt2] += g.aw == 4 && g.kt == 2;
    reached[kAw4Kt4] += g.aw == 4 && g.kt == 4;
    reached[kTail] += p.tail;
    reached[kScalar] += g.vec == 1;
    reached[kTapGroups] += p.groups > 1;
    reached[kAlignHead] += a.align_head != 0;
    reached[kBitTables] += a.code_bits != nullptr;
    reached[kBlocksPerWg] += a.blocks_per_wg > 1;
    bool deep = false, copy = false;
    for (int i = 0; i < p.groups; ++i) deep |= p.cfg[i].depth == 2, copy |= p.a[i].rep_copy_stride > 0;
    reached[kDepth2] += deep;
    reached[kReplicaCopy] += copy;
}

// Every launch of an accepted plan against the kernels' contract (with what the enqueue adds: the uploaded records, the scratch),
// and every tap of the call in exactly one launch with its caller's index
void check_plan(const Case &c, CorrPlan &p, const char *what)
{
    std::vector<int> seen((size_t)c.L, 0);
    auto own = [&](int index, int shift) {
        const bool in = index >= 0 && index < c.L && c.shifts[(size_t)index] == shift;
        CHECK(in, "%s: a launch takes tap %d at shift %d", what, index, shift);
        if (in) ++seen[(size_t)index];
    };
    float *const scratch = addr<float>(0xb00000000000ull);
    if (p.kind) {
        if (!p.m.params) p.m.params = addr<const gat_channel_params>(0x800000000000ull);
        p.m.partial = scratch;
        if (p.kind == 2) check_mfma_bf16(p.m, p.rt, p.nct, c.sig.layout, p.grid, p.lds, broken);
        else check_mfma(p.m, p.nct, p.grid, p.lds, broken);
        for (int l = 0; l < p.m.L && l < kMfmaMaxTaps; ++l) own(p.m.tap_index[l], p.m.shifts[l]);
        CHECK(p.splits == p.m.splits && p.info.matrix_core == p.kind && p.info.workgroups == (int32_t)p.grid, "%s: matrix plan and launch info", what);
        // host records that a matrix kernel would poison for its own wrap rule never reach one
        if (const CorrCall call = c.call(); call.params_inline)
            for (long long i = 0; i < (long long)c.B * c.K; ++i) {
                const double ratio = call.params_inline[i].code_freq_hz / c.fs;
                CHECK(!mfma_wrap_bad(ratio, c.tab.Lc), "%s: record %lld (ratio %g, %d chips) given to matrix kernel %d", what, i, ratio, c.tab.Lc, p.kind);
                matrix_records_checked += 1;
            }
    } else {
        CHECK(p.groups >= 1 && p.groups <= c.L, "%s: %d tap groups", what, p.groups);
        for (int g = 0; g < p.groups; ++g) {
            p.a[g].partial = scratch;
            check_dc(p.a[g], p.cfg[g], false, broken);
            for (int l = 0; l < p.cfg[g].taps && l < kMaxTapsPerLaunch; ++l) own(p.a[g].tap_index[l], p.a[g].shifts[l]);
            CHECK(p.a[g].splits == p.splits && p.a[g].Ltot == c.L, "%s: group %d splits %d of %d", what, g, p.a[g].splits, p.splits);
        }
        CHECK(p.tail == (p.cfg[0].vec == 4 && c.sig.num_samples % layout_vec_samples(c.sig.layout) != 0), "%s: tail", what);
    }
    CHECK(p.finalize == (p.splits > 1 && !(c.flags & GAT_FLAG_ATOMIC)), "%s: finalize %d with %d splits", what, (int)p.finalize, p.splits);
    for (int l = 0; l < c.L; ++l) CHECK(seen[(size_t)l] == 1, "%s: tap %d is in %d launches", what, l, seen[(size_t)l]);
}

Refusal plan_case(const Case &c, CorrPlan &p)
{
    const CorrCall call = c.call();
    const Refusal r = corr_check_call(c.tab, call);
    return r.code != GAT_OK ? r : corr_plan(c.knobs, c.tab, call, p);
}
Refusal plan_resident_case(const Case &c, long long wgs, DcArgs *a, DcLaunch *cfg)
{
    return corr_plan_resident(c.knobs, c.tab, &c.sig, c.K, c.L, c.shifts.data(), c.fs, wgs, a, cfg);
}

// ---- refusals: each message of the header with its code, from a valid call ------------------------------------------------------
struct Refused {
    Case c;
    bool resident; // through corr_plan_resident (64 workgroups)
    int code;
    const char *msg;
};
std::vector<Refused> refusal_cases()
{
    std::vector<Refused> out;
    const Case ok = bench_case(GAT_LAYOUT_PLANAR, 1023, 1.023e6, 20000, 4, 3, 2, 2, 1, true);
    out.push_back({ok, false, GAT_OK, nullptr}); // (the valid call itself)
    auto refused = [&](const Case &t, int code, const char *msg) { out.push_back({t, false, code, msg}); };
    Case t = ok;
    t.tab.d_codes = nullptr, refused(t, GAT_ERR_STATE, "gat_set_codes has not been called");
    t = ok, t.sig.layout = 4, refused(t, GAT_ERR_ARG, "unknown signal layout");
    t = ok, t.sig.im = nullptr, refused(t, GAT_ERR_ARG, "signal pointers do not match the layout");
    t = ok, t.sig.layout = GAT_LAYOUT_INTERLEAVED_I8, refused(t, GAT_ERR_ARG, "signal pointers do not match the layout");
    t = ok, t.K = 0, refused(t, GAT_ERR_ARG, "sizes must be positive");
    t = ok, t.sig.num_samples = 0, refused(t, GAT_ERR_ARG, "sizes must be positive");
    t = ok, t.L = GAT_MAX_TAPS + 1, t.shifts.resize((size_t)t.L), refused(t, GAT_ERR_RANGE, "num_taps outside 1..GAT_MAX_TAPS");
    t = ok, t.fs = 0.0, refused(t, GAT_ERR_ARG, "sampling frequency must be positive");
    t = ok, t.fs = INFINITY, refused(t, GAT_ERR_ARG, "sampling frequency must be positive");
    t = ok, t.flags = GAT_FLAG_GRAPH, refused(t, GAT_ERR_ARG, "unknown flag bits");
    t = ok, t.shifts[0] = -((1 << 30) - 20000), refused(t, GAT_ERR_RANGE, "num_samples + |shift| must stay below 2^30");
    t = ok, t.sig.block_stride = -1, refused(t, GAT_ERR_ARG, "negative stride");
    // the plan's own: a grid beyond 2^31 workgroups of either kernel family, tables and tap spans beyond a workgroup's LDS
    t = ok, t.host = false, t.B = 1 << 30, t.K = 4, refused(t, GAT_ERR_RANGE, "grid too large");
    t = bench_case(GAT_LAYOUT_PLANAR, 1023, 1.023e6, 64, 16, 3, 64, 1 << 30, GAT_MC_BF16_SPLIT, false), refused(t, GAT_ERR_RANGE, "grid too large");
    t = ok, t.tab = tables(200000, false, 256), refused(t, GAT_ERR_RANGE, "code table too long for the LDS-resident chip table of the vector kernel");
    // (two antennas of int8 pairs: steps of 2048 samples, where the widest tap span needs more room than the default segment)
    t = bench_case(GAT_LAYOUT_INTERLEAVED_I8, 135000, 1.023e6, 20000, 2, 3, 2, 2, 1, true), t.tab = tables(135000, false, 256), t.shifts = {-1024, 0, 1024};
    refused(t, GAT_ERR_RANGE, "tap span and code table do not fit the LDS of one workgroup");
    // (within the options' ranges every shape has an instance -- 4 antennas x 8 taps is one --: a tile beyond kMaxAntTile has none)
    t = ok, t.sig.num_ants = 7, t.knobs.max_ant_tile = 7, refused(t, GAT_ERR_UNSUPPORTED, "no kernel instance for this shape");
    // the resident correlator's.  Its last two ("no instance for this geometry", "no kernel instance for this shape") guard what
    // plan_vector never gives a resident call -- two sample sets, one-wave workgroups, a tile without an instance -- and cannot be reached
    auto res_refused = [&](const Case &u, int code, const char *msg) { out.push_back({u, true, code, msg}); };
    const Case res = bench_case(GAT_LAYOUT_PLANAR, 1023, 1.023e6, 20000, 4, 3, 2, 1, 1, true);
    res_refused(res, GAT_OK, nullptr);
    t = res, t.tab.d_codes = nullptr, res_refused(t, GAT_ERR_STATE, "gat_set_codes has not been called");
    t = res, t.shifts = {-3000, 0, 3000}, res_refused(t, GAT_ERR_UNSUPPORTED, "resident correlator: the taps need more than one launch");
    const char *const align = "resident correlator: block starts must be 16-byte aligned and num_samples a multiple of the load group";
    t = res, t.sig.num_samples = 19999, res_refused(t, GAT_ERR_UNSUPPORTED, align);
    t = res, t.sig.ant_stride = 20001, res_refused(t, GAT_ERR_UNSUPPORTED, align);
    return out;
}
long refusals_seen = 0;
void refusals()
{
    for (const Refused &x : refusal_cases()) {
        CorrPlan p;
        DcArgs a;
        DcLaunch cfg;
        const Refusal r = x.resident ? plan_resident_case(x.c, 64, &a, &cfg) : plan_case(x.c, p);
        const bool same = r.code == x.code && (x.msg ? r.msg && std::strcmp(r.msg, x.msg) == 0 : !r.msg);
        CHECK(same, "%s%s: got %d (%s)", x.resident ? "resident: " : "", x.msg ? x.msg : "the valid call", r.code, r.msg ? r.msg : "none");
        refusals_seen += x.code != GAT_OK;
    }
}

// ---- the random sweep -------------------------------------------------------------------------------------------------------------
long planned = 0, refused_calls = 0, resident_planned = 0;
void sweep(int calls)
{
    for (int it = 0; it < calls; ++it) {
        const Case c = random_case();
        CorrPlan p;
        const Refusal r = plan_case(c, p);
        if (r.code == GAT_OK) {
            ++planned;
            count_branches(p);
            check_plan(c, p, "sweep");
        } else { // (a valid call: only what the tables and taps can make too large for a workgroup's LDS)
            ++refused_calls;
            CHECK(r.code == GAT_ERR_RANGE && r.msg, "sweep: refused with %d (%s)", r.code, r.msg ? r.msg : "none");
        }
        if (c.B != 1 || c.K > kResMaxChannels) continue;
        DcArgs a;
        DcLaunch cfg;
        const Refusal rr = plan_resident_case(c, pick<long long>({8, 64, 128}), &a, &cfg);
        if (rr.code == GAT_OK) {
            ++resident_planned;
            check_dc(a, cfg, true, broken);
            CHECK(a.keep_l2 == 0 && cfg.taps == c.L, "sweep: resident launch");
        } else {
            CHECK((rr.code == GAT_ERR_UNSUPPORTED || rr.code == GAT_ERR_RANGE) && rr.msg, "sweep: resident call refused with %d", rr.code);
        }
    }
}

// ---- the matrix kernels' wrap rule: a call with inline host records goes to a matrix kernel only if none breaks mfma_wrap_bad --------
void wrap_rule()
{
    for (int mode : {(int)GAT_MC_F32, (int)GAT_MC_BF16_SPLIT})
        for (int K : {1, 2, 4})
            for (int L : {6, 8, 16}) {
                Case c = bench_case(GAT_LAYOUT_PLANAR, 1023, 1.023e6, 20000, 16, L, K, 1, mode, true);
                const double edge = c.fs * 1023.0 / 32.0; // code frequency at which 32 samples span the table
                for (double f : {1.023e6, std::nextafter(edge, 0.0), edge, std::nextafter(edge, INFINITY), 1.5 * edge}) {
                    c.recs[(size_t)K - 1].code_freq_hz = f;
                    CorrPlan p;
                    const Refusal r = plan_case(c, p);
                    const bool bad = mfma_wrap_bad(f / c.fs, 1023);
                    CHECK(r.code == GAT_OK && (p.kind != 0) == !bad, "wrap rule: mode %d, %d channels, %d taps, code frequency %.17g: status %d, kind %d", mode, K, L, f, r.code, p.kind);
                    if (r.code == GAT_OK) check_plan(c, p, "wrap rule");
                }
            }
}

// ---- pinned rows: the benchmark's shapes at 256 CUs ------------------------------------------------------------------------------
struct Row {
    int kind, MT, aw, kt, nw, depth, vec, splits, bpw, seg_steps, lds;
    unsigned grid;
    int rt, nct, nslots, mb_mode; // kind 2
};
Row row_of(const CorrPlan &p)
{
    if (p.kind) return {p.kind, 0, 0, 0, 0, 0, 4, p.splits, 1, 0, (int)p.lds, p.grid, p.rt, p.nct, p.m.nslots, p.m.mb_mode};
    const DcArgs &a = p.a[0];
    const DcLaunch &g = p.cfg[0];
    return {0, g.ant_tile, g.aw, g.kt, g.nw, g.depth, g.vec, p.splits, a.blocks_per_wg, a.seg_steps, (int)g.lds_bytes, g.grid, 0, 0, 0, 0};
}
constexpr int kPinned = 8;
const char *const kPinnedName[kPinned] = {"configs[1]", "configs[2]", "configs[3]", "configs[4]", "configs[1] int16", "configs[1] int8", "single block", "64 x 32 int16"};
Case pinned_case(int i)
{
    const double l1 = 1.023e6, l5 = 10.23e6;
    switch (i) {
    case 0: return bench_case(GAT_LAYOUT_PLANAR, 1023, l1, 20000, 4, 3, 1, 4096, GAT_MC_AUTO, false);
    case 1: return bench_case(GAT_LAYOUT_PLANAR, 10230, l5, 50000, 4, 5, 12, 1024, GAT_MC_AUTO, false);
    case 2: return bench_case(GAT_LAYOUT_PLANAR, 1023, l1, 50000, 16, 3, 4, 512, GAT_MC_AUTO, false);
    case 3: return bench_case(GAT_LAYOUT_PLANAR, 1023, l1, 2000000, 64, 3, 64, 1, GAT_MC_AUTO, false, 20e-3);
    case 4: return bench_case(GAT_LAYOUT_INTERLEAVED_I16, 1023, l1, 20000, 4, 3, 1, 4096, GAT_MC_AUTO, false);
    case 5: return bench_case(GAT_LAYOUT_INTERLEAVED_I8, 1023, l1, 20000, 4, 3, 1, 4096, GAT_MC_AUTO, false);
    case 6: return bench_case(GAT_LAYOUT_PLANAR, 1023, l1, 20000, 4, 3, 1, 1, GAT_MC_AUTO, true);
    default: return bench_case(GAT_LAYOUT_INTERLEAVED_I16, 1023, l1, 50000, 64, 3, 32, 16, GAT_MC_AUTO, false);
    }
}
// kind, MT, aw, kt, nw, depth, vec, splits, blocks_per_wg, seg_steps, lds_bytes, grid, rt, nct, nslots, mb_mode
const Row kPinnedRow[kPinned] = {
    {0, 4, 1, 1, 4, 2, 4, 1, 1, 8, 38464, 4096u, 0, 0, 0, 0},    // configs[1]: depth 2
    {0, 2, 2, 2, 4, 1, 4, 1, 1, 7, 40608, 6144u, 0, 0, 0, 0},    // configs[2]: the 2 x 2 tile
    {0, 4, 4, 4, 4, 1, 4, 1, 1, 8, 55552, 512u, 0, 0, 0, 0},     // configs[3]
    {2, 0, 0, 0, 0, 0, 4, 256, 1, 0, 154736, 768u, 4, 4, 23, 0}, // configs[4]: split-bf16, three terms
    {0, 4, 1, 1, 4, 1, 4, 1, 1, 8, 38464, 4096u, 0, 0, 0, 0},    // configs[1] int16
    {0, 4, 1, 1, 4, 1, 4, 1, 1, 4, 38464, 4096u, 0, 0, 0, 0},    // configs[1] int8
    {0, 4, 1, 1, 4, 1, 4, 20, 1, 1, 38464, 24u, 0, 0, 0, 0},     // single block
    {2, 0, 0, 0, 0, 0, 4, 16, 1, 0, 116880, 768u, 4, 2, 12, 2},  // 64 x 32 int16: split-bf16, two terms
};
void pinned()
{
    for (int i = 0; i < kPinned; ++i) {
        const Case c = pinned_case(i);
        CorrPlan p;
        const Refusal r = plan_case(c, p);
        CHECK(r.code == GAT_OK, "%s: refused (%s)", kPinnedName[i], r.msg ? r.msg : "none");
        if (r.code != GAT_OK) continue;
        check_plan(c, p, kPinnedName[i]);
        const Row got = row_of(p), &w = kPinnedRow[i];
        CHECK(std::memcmp(&got, &w, sizeof got) == 0,
              "%s: {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %uu, %d, %d, %d, %d}, pinned {%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %uu, %d, %d, %d, %d}", kPinnedName[i],
              got.kind, got.MT, got.aw, got.kt, got.nw, got.depth, got.vec, got.splits, got.bpw, got.seg_steps, got.lds, got.grid, got.rt, got.nct, got.nslots,
              got.mb_mode, w.kind, w.MT, w.aw, w.kt, w.nw, w.depth, w.vec, w.splits, w.bpw, w.seg_steps, w.lds, w.grid, w.rt, w.nct, w.nslots, w.mb_mode);
    }
}

} // namespace

int main()
{
    refusals();
    pinned();
    sweep(6000);
    wrap_rule();
    for (int b = 0; b < kBranches; ++b) {
        std::printf("  %-40s %ld\n", kBranchName[b], reached[b]);
        CHECK(reached[b] > 0, "no call of the sweep reached: %s", kBranchName[b]);
    }
    std::printf("  %-40s %ld\n", "host records given to a matrix kernel", matrix_records_checked);
    CHECK(matrix_records_checked > 0, "no call gave inline host records to a matrix kernel");
    std::printf("pinned %d plans\n", kPinned);
    std::printf("planned %ld calls (%ld refused, %ld resident plans), %ld refusals provoked, %d failures\n", planned, refused_calls, resident_planned, refusals_seen, failures);
    return failures ? 1 : 0;
}
