// Stand-alone check of the carrier smoothing's pure plan (csrc/gat_smooth_plan.h) and of the host twin's loops over it (sm_host_run,
// the rule of csrc/gat_smooth.h).  Every documented refusal must return its code with nothing planned; random plans must put every
// (epoch, channel) into exactly one thread of the chunk stages and one of the output stage, the scratch regions must not overlap; the
// segment combine must be associative on random triples and agree with pushing the epochs one by one.  The twin then runs on heap
// buffers of exactly the extents the call describes -- every subset of the optional outputs, with and without Doppler and mask -- so
// that AddressSanitizer sees any access outside them, and the four stages of the device split, walked here in plain loops over the
// same plan (runs, chunk segments, the channels' scan with one, two and three chunks a lane, emit, output), must give the twin's
// bytes.  Last, hostile entries: NaN, the infinities, the largest finite values and the integer extremes in every input; everything
// must stay defined (the sanitizers' business, float-cast-overflow among them) and no channel may touch another.  Built with
// -fsanitize=address,undefined,float-cast-overflow by tests/test_smoothing_plan_host.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "gat_smooth_plan.h"

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

const double kInf = std::numeric_limits<double>::infinity();
const double kNaN = std::numeric_limits<double>::quiet_NaN();
template <class T>
T *given()
{
    return reinterpret_cast<T *>(uintptr_t(0x9000));
}

gat_smooth_config sm_cfg(int W = 100, bool rate = false)
{
    gat_smooth_config c{};
    c.struct_size = sizeof(gat_smooth_config);
    c.flags = rate ? GAT_SMOOTH_RATE_TEST : 0;
    c.window = W;
    c.carrier_hz = 1575.42e6, c.if_hz = 1234.5, c.epoch_seconds = 0.02, c.cmc_gate_s = 15.0 / 299792458.0;
    c.rate_gate_cycles = rate ? 0.5 : 0.0;
    return c;
}
SmCall call(int E, int K, const gat_smooth_config *cfg)
{
    SmCall a{};
    a.in = SmIn{given<int32_t>(), given<double>(), given<int32_t>(), given<double>(), given<int64_t>(), given<double>(), given<double>(), nullptr};
    a.E = E, a.K = K, a.cfg = cfg;
    a.out.tx_frac_out = given<double>();
    return a;
}

void expect_refusal(const SmCall &a, int code, const char *what)
{
    SmPlan p, q;
    std::memset(&p, 0x5a, sizeof p);
    std::memset(&q, 0x5a, sizeof q);
    const Refusal r = sm_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_smooth_config good = sm_cfg(), rated = sm_cfg(100, true);
    SmCall a = call(3, 6, &good);
    a.in.tx_ms = nullptr, expect_refusal(a, GAT_ERR_ARG, "null tx_ms"), a.in.tx_ms = given<int32_t>();
    a.in.tx_frac = nullptr, expect_refusal(a, GAT_ERR_ARG, "null tx_frac"), a.in.tx_frac = given<double>();
    a.in.rx_ms = nullptr, expect_refusal(a, GAT_ERR_ARG, "null rx_ms"), a.in.rx_ms = given<int32_t>();
    a.in.rx_frac = nullptr, expect_refusal(a, GAT_ERR_ARG, "null rx_frac"), a.in.rx_frac = given<double>();
    a.in.cycles = nullptr, expect_refusal(a, GAT_ERR_ARG, "null carrier_cycles"), a.in.cycles = given<int64_t>();
    a.in.cfrac = nullptr, expect_refusal(a, GAT_ERR_ARG, "null carrier_frac"), a.in.cfrac = given<double>();
    a.out.tx_frac_out = nullptr, expect_refusal(a, GAT_ERR_ARG, "null tx_frac_out"), a.out.tx_frac_out = given<double>();
    SmPlan p{};
    a.in.doppler = nullptr;
    CHECK(sm_plan(a, &p).code == GAT_OK, "no doppler without the rate test");
    a.cfg = &rated;
    expect_refusal(a, GAT_ERR_ARG, "the rate test without doppler");
    expect_refusal(call(3, 6, nullptr), GAT_ERR_ARG, "null config");
    CHECK(sm_plan(call(3, 6, &good), nullptr).code == GAT_ERR_ARG, "null plan");
    gat_smooth_config c = good;
    c.struct_size += 8;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "struct_size");
    for (uint32_t f : {2u, 3u, 0x80000000u}) {
        c = rated, c.flags = f;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "flags");
    }
    c = good, c.reserved = 1;
    expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "reserved");
    for (double v : {kNaN, kInf, -kInf, 0.0, -0.0, -1.0}) {
        c = good, c.carrier_hz = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "carrier_hz");
        c = good, c.epoch_seconds = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "epoch_seconds");
    }
    for (double v : {kNaN, kInf, -kInf}) {
        c = good, c.if_hz = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_ARG, "if_hz");
    }
    expect_refusal(call(0, 6, &good), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(3, 0, &good), GAT_ERR_ARG, "K = 0");
    expect_refusal(call(-1, 6, &good), GAT_ERR_ARG, "E = -1");
    for (int w : {0, -1, 65537, 0x7fffffff}) {
        c = good, c.window = w;
        expect_refusal(call(3, 6, &c), GAT_ERR_RANGE, "window");
    }
    for (double v : {kNaN, kInf, -kInf, 0.0, -1e-9, std::nextafter(0x1p-18, 1.0)}) {
        c = good, c.cmc_gate_s = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_RANGE, "cmc_gate_s");
    }
    for (double v : {kNaN, kInf, -kInf, 0.0, -0.5}) {
        c = rated, c.rate_gate_cycles = v;
        expect_refusal(call(3, 6, &c), GAT_ERR_RANGE, "rate_gate_cycles");
        c = good, c.rate_gate_cycles = v; // not read without the rate test
        CHECK(sm_plan(call(3, 6, &c), &p).code == GAT_OK, "rate_gate_cycles read without the rate test");
    }
    expect_refusal(call(3, GAT_MAX_FIX_CHANNELS + 1, &good), GAT_ERR_RANGE, "K = 65");
    expect_refusal(call(GAT_MAX_SMOOTH_EPOCHS + 1, 6, &good), GAT_ERR_RANGE, "E = 2^20 + 1");
    expect_refusal(call(GAT_MAX_SMOOTH_EPOCHS, 64, &good), GAT_ERR_RANGE, "scratch above 1 GiB");
    c = good, c.window = 65536, c.cmc_gate_s = 0x1p-18;
    CHECK(sm_plan(call(GAT_MAX_SMOOTH_EPOCHS, 48, &c), &p).code == GAT_OK && (long long)p.bytes <= kSmMaxScratch, "the largest call");
}

int plans(std::mt19937_64 &rng, int count)
{
    const gat_smooth_config cfg = sm_cfg();
    for (int n = 0; n < count; ++n) {
        const bool small = n < 40 || n % 8 == 0;
        const int K = 1 + (int)(rng() % GAT_MAX_FIX_CHANNELS);
        const int E = n < 40 ? n + 1 : (small ? 1 + (int)(rng() % 3000) : 1 + (int)(rng() % (K > 48 ? 700000 : GAT_MAX_SMOOTH_EPOCHS)));
        SmPlan p{};
        CHECK(sm_plan(call(E, K, &cfg), &p).code == GAT_OK, "E %d K %d refused", E, K);
        CHECK(p.E == E && p.K == K && p.cells == (long long)E * K && p.chunks == (E + kSmChunk - 1) / kSmChunk, "geometry");
        CHECK(p.lanes >= K && p.lanes < 2 * K && (p.lanes & (p.lanes - 1)) == 0 && p.rows * p.lanes == kSmThreads && p.rows * p.run == kSmChunk, "split");
        CHECK(p.out_groups == (p.cells + kSmThreads - 1) / kSmThreads && p.chan_groups == (K + kSmChanWaves - 1) / kSmChanWaves, "groups");
        CHECK(p.off_totals == 0 && p.off_runs >= (size_t)p.chunks * K * sizeof(SmSeg) && p.off_C >= p.off_runs + (size_t)p.chunks * kSmThreads * sizeof(SmSeg) &&
                  p.off_SS >= p.off_C + (size_t)p.cells * 8 && p.off_arc >= p.off_SS + (size_t)p.cells * 8 && p.bytes >= p.off_arc + (size_t)p.cells * 4 &&
                  (long long)p.bytes <= kSmMaxScratch && (p.off_runs | p.off_C | p.off_SS | p.off_arc) % 16 == 0,
              "scratch layout");
        gat_smooth_plan rep{};
        sm_report(p, &rep);
        CHECK(rep.chunk_epochs == kSmChunk && rep.num_chunks == p.chunks && rep.lanes == p.lanes && rep.rows == p.rows && rep.run_epochs == p.run &&
                  rep.threads == kSmThreads && rep.lds_bytes == kSmLdsBytes && rep.chunk_workgroups == p.chunks && rep.channel_workgroups == p.chan_groups &&
                  rep.output_workgroups == p.out_groups && rep.scratch_bytes == (int64_t)p.bytes && rep.struct_size == sizeof rep,
              "report");
        int e = -1, k = -1;
        if (small) { // every thread of both grids: each (epoch, channel) once
            std::vector<uint8_t> chunked((size_t)E * K, 0), flat((size_t)E * K, 0);
            for (int c = 0; c < p.chunks; ++c)
                for (int t = 0; t < kSmThreads; ++t) {
                    int lane, row, e0, e1;
                    sm_thread(p.lanes, t, &lane, &row);
                    CHECK(lane >= 0 && lane < p.lanes && row >= 0 && row < p.rows && row * p.lanes + lane == t, "a thread outside the workgroup");
                    if (!(lane < K && sm_run(E, p.run, c, row, &e0, &e1))) continue;
                    CHECK(e0 >= c * kSmChunk && e1 <= E && e1 <= (c + 1) * kSmChunk && e0 < e1, "a run outside its chunk");
                    for (int i = e0; i < e1 && i < E; ++i) chunked[(size_t)i * K + lane] += 1;
                }
            for (long long g = 0; g < p.out_groups; ++g)
                for (int lane = 0; lane < kSmThreads; ++lane)
                    if (sm_unit(g, lane, p.cells, K, &e, &k)) {
                        CHECK(e >= 0 && e < E && k >= 0 && k < K, "a thread outside the call");
                        if (e >= 0 && e < E && k >= 0 && k < K) flat[(size_t)e * K + k] += 1;
                    }
            for (size_t i = 0; i < chunked.size(); ++i) CHECK(chunked[i] == 1 && flat[i] == 1, "E %d K %d: a cell is covered %d and %d times", E, K, chunked[i], flat[i]);
        } else {
            const int last = (int)((p.cells - 1) % kSmThreads);
            CHECK(sm_unit(p.out_groups - 1, last, p.cells, K, &e, &k) && e == E - 1 && k == K - 1, "the last cell");
            CHECK(!sm_unit(p.out_groups, 0, p.cells, K, &e, &k), "a workgroup past the last");
            int e0, e1, covered = 0;
            for (int r = 0; r < p.rows; ++r)
                if (sm_run(E, p.run, p.chunks - 1, r, &e0, &e1)) covered += e1 - e0;
            CHECK(covered == E - (p.chunks - 1) * kSmChunk && !sm_run(E, p.run, p.chunks, 0, &e0, &e1), "the last chunk");
        }
    }
    return count;
}

bool seg_equal(const SmSeg &a, const SmSeg &b)
{
    return a.Q == b.Q && a.S == b.S && a.len == b.len && a.reset == b.reset && std::memcmp(a.cnt, b.cnt, sizeof a.cnt) == 0;
}

// (a b) c = a (b c) on random segments, sums near the wrap among them; a combine of pushed runs is the run pushed whole
void combine(std::mt19937_64 &rng)
{
    for (int n = 0; n < 20000; ++n) {
        SmSeg s[3];
        int e = 0;
        for (SmSeg &x : s) {
            x = sm_empty();
            if (n % 2) { // any values
                x.Q = rng(), x.S = rng(), x.len = (int32_t)(rng() % 100000), x.reset = (int32_t)(rng() % 1000000) - 1;
                for (int32_t &c : x.cnt) c = (int32_t)(rng() % 100000);
            } else { // pushed epochs
                const int len = (int)(rng() % 6);
                for (int i = 0; i < len; ++i, ++e) {
                    const int st = (int)(rng() % 16);
                    sm_push(&x, e, sm_arc_start(st) || !(st & 1) ? 0 : (int64_t)(rng() % (1u << 31)) - (1 << 30), st & 1 ? st : 0);
                }
            }
        }
        const SmSeg left = sm_combine(sm_combine(s[0], s[1]), s[2]), right = sm_combine(s[0], sm_combine(s[1], s[2]));
        CHECK(seg_equal(left, right), "the combine is not associative");
        CHECK(seg_equal(sm_combine(sm_empty(), s[1]), s[1]) && seg_equal(sm_combine(s[1], sm_empty()), s[1]), "the empty segment is not neutral");
    }
    // a run pushed whole against its pieces combined
    for (int n = 0; n < 2000; ++n) {
        const int len = 1 + (int)(rng() % 40), cut1 = (int)(rng() % (len + 1)), cut2 = cut1 + (int)(rng() % (len - cut1 + 1));
        SmSeg whole = sm_empty(), a = sm_empty(), b = sm_empty(), c = sm_empty();
        for (int e = 0; e < len; ++e) {
            const int st = (int)(rng() % 16) | 1;
            const int64_t q = sm_arc_start(st) ? 0 : (int64_t)(rng() % (1u << 31)) - (1 << 30);
            sm_push(&whole, e, q, st);
            sm_push(e < cut1 ? &a : e < cut2 ? &b : &c, e, q, st);
        }
        CHECK(seg_equal(sm_combine(sm_combine(a, b), c), whole), "pieces combined differ from the whole run");
    }
}

// ---- the twin on exact buffers --------------------------------------------------------------------------------------------------------
struct Buffers {
    int E, K;
    std::unique_ptr<int32_t[]> tx_ms, rx_ms;
    std::unique_ptr<double[]> tx_frac, rx_frac, cfrac, doppler;
    std::unique_ptr<int64_t[]> cycles;
    std::unique_ptr<uint8_t[]> valid;
    Buffers(int E_, int K_) : E(E_), K(K_)
    {
        const size_t n = (size_t)E * K;
        tx_ms.reset(new int32_t[n]), rx_ms.reset(new int32_t[E]), tx_frac.reset(new double[n]), rx_frac.reset(new double[E]);
        cfrac.reset(new double[n]), doppler.reset(new double[n]), cycles.reset(new int64_t[n]), valid.reset(new uint8_t[n]);
    }
    SmIn in(bool with_doppler, bool with_valid) const
    {
        return SmIn{tx_ms.get(), tx_frac.get(), rx_ms.get(), rx_frac.get(), cycles.get(), cfrac.get(), with_doppler ? doppler.get() : nullptr,
                    with_valid ? valid.get() : nullptr};
    }
};

// a consistent case: travel time linear in time, the carrier its mirror, noise on the code, slips, gaps and a mask
void fill(Buffers &b, std::mt19937_64 &rng, const gat_smooth_config &cfg, bool week_wrap)
{
    std::uniform_real_distribution<double> uni(0.0, 1.0);
    std::normal_distribution<double> gauss(0.0, 1.0);
    const int step = 20;
    const int64_t rx0 = week_wrap ? kObsWeekMs - 7 * step - 3 : 244804321;
    for (int e = 0; e < b.E; ++e) b.rx_ms[e] = (int32_t)((rx0 + (int64_t)step * e) % kObsWeekMs), b.rx_frac[e] = 0.000123456;
    for (int k = 0; k < b.K; ++k) {
        const double rho0 = 0.066 + 0.02 * uni(rng), v = (uni(rng) - 0.5) * 5e-6;
        long long amb = (long long)(rng() % 2000000000ull) - 1000000000ll;
        for (int e = 0; e < b.E; ++e) {
            const size_t o = (size_t)e * b.K + k;
            const double t = e * cfg.epoch_seconds, rho = rho0 + v * t;
            const double off = b.rx_frac[e] - rho, m = std::floor(off * 1e3);
            double frac = off - m * 1e-3;
            b.tx_ms[o] = (int32_t)obs_mod((int64_t)b.rx_ms[e] + (int64_t)m, kObsWeekMs);
            if (rng() % 50 == 0) amb += 300; // a slip
            const long double phase = (long double)cfg.if_hz * cfg.epoch_seconds * e - (long double)cfg.carrier_hz * rho;
            const long double whole = std::floor(phase);
            b.cycles[o] = (int64_t)whole + amb, b.cfrac[o] = (double)(phase - whole);
            b.tx_frac[o] = frac + gauss(rng) * 2e-9;
            b.doppler[o] = -cfg.carrier_hz * v;
            b.valid[o] = rng() % 40 == 0 ? 0 : (uint8_t)(1 + rng() % 255);
            if (rng() % 60 == 0) b.tx_ms[o] = -1;
        }
    }
}

struct Outputs {
    std::unique_ptr<double[]> tx, cmc;
    std::unique_ptr<int32_t[]> count;
    std::unique_ptr<uint8_t[]> status;
    std::unique_ptr<gat_smooth_channel[]> chan;
    SmOut out{};
    Outputs(int E, int K, int subset) // bit 0: count, 1: cmc_s, 2: status, 3: channels
    {
        const size_t n = (size_t)E * K;
        tx.reset(new double[n]), out.tx_frac_out = tx.get();
        std::memset(tx.get(), 0x5a, n * sizeof(double));
        if (subset & 1) count.reset(new int32_t[n]), out.count = count.get(), std::memset(count.get(), 0x5a, n * 4);
        if (subset & 2) cmc.reset(new double[n]), out.cmc_s = cmc.get(), std::memset(cmc.get(), 0x5a, n * 8);
        if (subset & 4) status.reset(new uint8_t[n]), out.status = status.get(), std::memset(status.get(), 0x5a, n);
        if (subset & 8) chan.reset(new gat_smooth_channel[K]), out.channels = chan.get(), std::memset(chan.get(), 0x5a, (size_t)K * sizeof(gat_smooth_channel));
    }
};
bool outputs_equal(const Outputs &a, const Outputs &b, int E, int K)
{
    const size_t n = (size_t)E * K;
    bool same = std::memcmp(a.tx.get(), b.tx.get(), n * 8) == 0;
    if (a.out.count && b.out.count) same = same && std::memcmp(a.count.get(), b.count.get(), n * 4) == 0;
    if (a.out.cmc_s && b.out.cmc_s) same = same && std::memcmp(a.cmc.get(), b.cmc.get(), n * 8) == 0;
    if (a.out.status && b.out.status) same = same && std::memcmp(a.status.get(), b.status.get(), n) == 0;
    if (a.out.channels && b.out.channels) same = same && std::memcmp(a.chan.get(), b.chan.get(), (size_t)K * sizeof(gat_smooth_channel)) == 0;
    return same;
}

// the four stages of the device split in plain loops, on a scratch of exactly the plan's bytes
void staged(const SmPlan &p, const SmIn &in, const SmOut &out)
{
    std::unique_ptr<char[]> scratch(new char[p.bytes]);
    std::memset(scratch.get(), 0x5a, p.bytes);
    SmSeg *totals = reinterpret_cast<SmSeg *>(scratch.get() + p.off_totals), *runs = reinterpret_cast<SmSeg *>(scratch.get() + p.off_runs);
    uint64_t *C = reinterpret_cast<uint64_t *>(scratch.get() + p.off_C), *SS = reinterpret_cast<uint64_t *>(scratch.get() + p.off_SS);
    int32_t *arc = reinterpret_cast<int32_t *>(scratch.get() + p.off_arc);
    const SmRule &r = p.rule;
    auto walk = [&](int lane, int e0, int e1, SmSeg s, bool emit) {
        SmEpoch prev = e0 > 0 ? sm_load(r, in, p.K, e0 - 1, lane) : SmEpoch{};
        for (int e = e0; e < e1; ++e) {
            const SmEpoch cur = sm_load(r, in, p.K, e, lane);
            int64_t q;
            const int st = sm_step(r, e == 0, prev, cur, &q);
            sm_push(&s, e, q, st);
            if (emit) {
                const size_t o = (size_t)e * p.K + lane;
                C[o] = s.Q, SS[o] = s.S, arc[o] = cur.measured ? s.reset : -1;
                if (out.status) out.status[o] = (uint8_t)st;
            }
            prev = cur;
        }
        return s;
    };
    for (int c = 0; c < p.chunks; ++c) { // chunk totals
        for (int t = 0; t < kSmThreads; ++t) {
            int lane, row, e0, e1;
            sm_thread(p.lanes, t, &lane, &row);
            SmSeg s = sm_empty();
            if (lane < p.K && sm_run(p.E, p.run, c, row, &e0, &e1)) s = walk(lane, e0, e1, s, false);
            runs[(size_t)c * kSmThreads + t] = s;
        }
        for (int k = 0; k < p.K; ++k) {
            SmSeg tot = sm_empty();
            for (int row = 0; row < p.rows; ++row) tot = sm_combine(tot, runs[(size_t)c * kSmThreads + row * p.lanes + k]);
            totals[(size_t)c * p.K + k] = tot;
        }
    }
    for (int k = 0; k < p.K; ++k) { // channel scan: 64 lanes of `per` chunks each, then the lanes' scan
        const int per = (p.chunks + kSmWave - 1) / kSmWave;
        SmSeg lane_seg[kSmWave], incl[kSmWave];
        for (int lane = 0; lane < kSmWave; ++lane) {
            const int c0 = lane * per < p.chunks ? lane * per : p.chunks, c1 = c0 + per < p.chunks ? c0 + per : p.chunks;
            lane_seg[lane] = sm_empty();
            for (int c = c0; c < c1; ++c) lane_seg[lane] = sm_combine(lane_seg[lane], totals[(size_t)c * p.K + k]);
            incl[lane] = lane_seg[lane];
        }
        for (int d = 1; d < kSmWave; d *= 2)
            for (int lane = kSmWave - 1; lane >= d; --lane) incl[lane] = sm_combine(incl[lane - d], incl[lane]);
        if (out.channels) out.channels[k] = gat_smooth_channel{incl[63].cnt[0], incl[63].cnt[1], incl[63].cnt[2], incl[63].cnt[3]};
        for (int lane = 0; lane < kSmWave; ++lane) {
            const int c0 = lane * per < p.chunks ? lane * per : p.chunks, c1 = c0 + per < p.chunks ? c0 + per : p.chunks;
            SmSeg run = lane ? incl[lane - 1] : sm_empty();
            for (int c = c0; c < c1; ++c) {
                const SmSeg v = totals[(size_t)c * p.K + k];
                totals[(size_t)c * p.K + k] = run;
                run = sm_combine(run, v);
            }
        }
    }
    for (int c = 0; c < p.chunks; ++c) // emit
        for (int t = 0; t < kSmThreads; ++t) {
            int lane, row, e0, e1;
            sm_thread(p.lanes, t, &lane, &row);
            if (!(lane < p.K && sm_run(p.E, p.run, c, row, &e0, &e1))) continue;
            SmSeg base = totals[(size_t)c * p.K + lane];
            for (int rr = 0; rr < row; ++rr) base = sm_combine(base, runs[(size_t)c * kSmThreads + rr * p.lanes + lane]);
            walk(lane, e0, e1, base, true);
        }
    for (long long g = 0; g < p.out_groups; ++g) // output
        for (int lane = 0; lane < kSmThreads; ++lane) {
            int e, k;
            if (!sm_unit(g, lane, p.cells, p.K, &e, &k)) continue;
            const size_t o = (size_t)e * p.K + k;
            const int a = arc[o], back = a < 0 ? -1 : e - sm_count(r, e, a);
            sm_emit(r, out, o, e, in.tx_frac[o], a, C[o], SS[o], back >= 0 ? SS[(size_t)back * p.K + k] : 0, a < 0 ? 0 : C[(size_t)a * p.K + k]);
        }
}

void twin(std::mt19937_64 &rng)
{
    // the last two: 66 and 129 chunks, where a lane of the channel scan holds two and three chunks and the lanes past the last idle
    const int shapes[][3] = {{1, 1, 1}, {2, 3, 1}, {255, 5, 7}, {256, 1, 256}, {257, 64, 2}, {3 * 256 + 7, 5, 259}, {3 * 256 + 7, 12, 65536}, {700, 33, 40},
                             {66 * 256 - 255, 5, 257}, {129 * 256 - 255, 5, 65536}};
    int runs = 0, deepest = 0;
    for (const auto &s : shapes) {
        const int E = s[0], K = s[1], W = s[2];
        for (int variant = 0; variant < 4; ++variant) { // bit 0: rate test and Doppler, bit 1: mask
            const bool rate = variant & 1, mask = variant & 2;
            const gat_smooth_config cfg = sm_cfg(W, rate);
            Buffers b(E, K);
            fill(b, rng, cfg, variant == 3);
            SmCall a{b.in(rate, mask), E, K, &cfg, SmOut{}};
            Outputs all(E, K, 15);
            a.out = all.out;
            SmPlan p{};
            CHECK(sm_plan(a, &p).code == GAT_OK, "E %d K %d refused", E, K);
            deepest = std::max(deepest, (p.chunks + kSmWave - 1) / kSmWave);
            sm_host_run(p, a.in, all.out);
            int measured = 0, arcs = 0, smoothed = 0;
            for (size_t i = 0; i < (size_t)E * K; ++i) measured += all.status[i] & 1, smoothed += all.count[i] > 1;
            for (int k = 0; k < K; ++k) arcs += all.chan[k].arcs;
            CHECK(measured > 0 && (E < 3 || arcs >= K) && (E < 20 || W < 2 || smoothed > 0), "E %d K %d: the case exercises nothing", E, K);
            for (int subset = 0; subset < 16; ++subset) {
                Outputs some(E, K, subset);
                sm_host_run(p, a.in, some.out);
                CHECK(outputs_equal(all, some, E, K), "E %d K %d subset %d: the twin's outputs depend on which are asked for", E, K, subset);
                ++runs;
            }
            Outputs dev(E, K, 15);
            staged(p, a.in, dev.out);
            CHECK(outputs_equal(all, dev, E, K), "E %d K %d W %d variant %d: the staged split differs from the twin", E, K, W, variant);
        }
    }
    CHECK(deepest == 3, "no plan gives a lane of the channel scan three chunks (%d)", deepest);
    std::printf("twin ran %d times on exact buffers, up to %d chunks a lane of the channel scan\n", runs, deepest);
}

// every input hostile in turn: everything stays defined, the staged split agrees, other channels keep their bytes
void hostile(std::mt19937_64 &rng)
{
    const int E = 300, K = 4;
    const gat_smooth_config cfg = sm_cfg(20, true);
    Buffers clean(E, K);
    fill(clean, rng, cfg, false);
    SmCall a{clean.in(true, true), E, K, &cfg, SmOut{}};
    Outputs base(E, K, 15);
    a.out = base.out;
    SmPlan p{};
    CHECK(sm_plan(a, &p).code == GAT_OK, "refused");
    sm_host_run(p, a.in, base.out);
    const double reals[] = {kNaN, kInf, -kInf, 1.7976931348623157e308, -1.7976931348623157e308, 4.9e-324, -0.0, 1e300, -1e18, 0x1p63, -0x1p63};
    const int64_t ints[] = {INT64_MAX, INT64_MIN, -1, 0, INT64_MAX - 1, INT64_MIN + 1};
    const int32_t smalls[] = {INT32_MAX, INT32_MIN, -1, 0, 604800000, 604799999, 302400000};
    int tried = 0;
    for (int field = 0; field < 7; ++field)
        for (int v = 0; v < 11; ++v) {
            Buffers b(E, K);
            const size_t n = (size_t)E * K;
            std::memcpy(b.tx_ms.get(), clean.tx_ms.get(), n * 4), std::memcpy(b.rx_ms.get(), clean.rx_ms.get(), (size_t)E * 4);
            std::memcpy(b.tx_frac.get(), clean.tx_frac.get(), n * 8), std::memcpy(b.rx_frac.get(), clean.rx_frac.get(), (size_t)E * 8);
            std::memcpy(b.cfrac.get(), clean.cfrac.get(), n * 8), std::memcpy(b.doppler.get(), clean.doppler.get(), n * 8);
            std::memcpy(b.cycles.get(), clean.cycles.get(), n * 8), std::memcpy(b.valid.get(), clean.valid.get(), n);
            const bool epoch_wide = field == 2 || field == 3;
            for (int hit = 0; hit < 3; ++hit) {
                const int e = (int)(rng() % E);
                const size_t o = (size_t)e * K + 1; // channel 1 alone
                if (field == 0) b.tx_ms[o] = smalls[v % 7];
                if (field == 1) b.tx_frac[o] = reals[v];
                if (field == 2) b.rx_ms[e] = smalls[v % 7];
                if (field == 3) b.rx_frac[e] = reals[v];
                if (field == 4) b.cycles[o] = ints[v % 6];
                if (field == 5) b.cfrac[o] = reals[v];
                if (field == 6) b.doppler[o] = reals[v];
            }
            Outputs got(E, K, 15), dev(E, K, 15);
            sm_host_run(p, b.in(true, true), got.out);
            staged(p, b.in(true, true), dev.out);
            CHECK(outputs_equal(got, dev, E, K), "field %d value %d: the staged split differs from the twin", field, v);
            if (!epoch_wide)
                for (int e = 0; e < E; ++e)
                    for (int k = 0; k < K; ++k) {
                        if (k == 1) continue;
                        const size_t o = (size_t)e * K + k;
                        CHECK(std::memcmp(&got.tx[o], &base.tx[o], 8) == 0 && got.count[o] == base.count[o] && got.status[o] == base.status[o] &&
                                  std::memcmp(&got.cmc[o], &base.cmc[o], 8) == 0,
                              "field %d value %d: channel %d changed with channel 1", field, v, k);
                    }
            for (size_t i = 0; i < n; ++i) CHECK(got.count[i] >= 0 && got.count[i] <= 20 && (got.status[i] & ~15) == 0, "an output outside its range");
            ++tried;
        }
    std::printf("hostile entries: %d cases\n", tried);
}

} // namespace

int main()
{
    std::mt19937_64 rng(20260);
    refusals();
    const int planned = plans(rng, 3000);
    combine(rng);
    twin(rng);
    hostile(rng);
    std::printf("planned %d calls, %d failures\n", planned, failures);
    return failures ? 1 : 0;
}
