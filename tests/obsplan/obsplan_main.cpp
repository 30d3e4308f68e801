// Stand-alone check of the observables' pure plan (csrc/gat_obs_plan.h) and of the host twin's loops over it (obs_host_run, the rule
// of csrc/gat_obs.h).  A few thousand random plans: walked through the workgroups, rows and lanes the kernels are launched with,
// every (block, channel) must be covered by exactly one run, every (epoch, channel) and every epoch's reception written exactly
// once, and the scratch regions must lie apart inside the reported bytes; every documented refusal must return its code with
// nothing planned.  The twin then runs on heap buffers of exactly the extents the call describes -- every output alone and all
// but each one -- so that AddressSanitizer sees any access outside them, and must find the transmit times the history was made
// from.  Built with -fsanitize=address,undefined by tests/test_observables_plan_host.py.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "gat_obs.h"
#include "gat_obs_plan.h"

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

gat_obs_config config()
{
    gat_obs_config c{};
    c.struct_size = sizeof(gat_obs_config);
    c.format = GAT_NAV_LNAV, c.code_length = 1023, c.symbol_blocks = 20;
    c.code_freq_nominal_hz = 1.023e6, c.block_seconds = 2046.0 / 2.046e6, c.sampling_freq_hz = 2.046e6, c.if_hz = 0.0;
    c.block_samples = 2046, c.max_frames = 3, c.min_tow_steps = 0, c.epoch_first = 0, c.epoch_stride = 1;
    c.rx_mode = GAT_OBS_RX_FROM_TX, c.travel_ms = 68, c.edge_margin = 0.1;
    return c;
}
ObsCall call(int B, int K, int E, const gat_obs_config *cfg)
{
    ObsOut o{};
    o.tx_ms = reinterpret_cast<int32_t *>(uintptr_t(0x9000));
    return ObsCall{kGiven, kGiven, kGiven, kGiven, B, K, E, cfg, o};
}

void expect_refusal(const ObsCall &a, int code, const char *what)
{
    ObsPlan p, q;
    std::memset(&p, 0x5a, sizeof p);
    std::memset(&q, 0x5a, sizeof q);
    const Refusal r = obs_plan(a, &p);
    CHECK(r.code == code, "%s: got %d, want %d", what, r.code, code);
    CHECK(std::memcmp(&p, &q, sizeof p) == 0, "%s: the plan was written", what);
}

void refusals()
{
    const gat_obs_config good = config();
    ObsCall a = call(100, 5, 101, &good);
    const void **ptrs[] = {&a.history, &a.mon, &a.nav, &a.frames};
    for (const void **p : ptrs) {
        *p = nullptr;
        expect_refusal(a, GAT_ERR_ARG, "null pointer");
        *p = kGiven;
    }
    a.out.tx_ms = nullptr;
    expect_refusal(a, GAT_ERR_ARG, "every output null");
    expect_refusal(call(100, 5, 101, nullptr), GAT_ERR_ARG, "null config");
    expect_refusal(call(0, 5, 1, &good), GAT_ERR_ARG, "B = 0");
    expect_refusal(call(100, 0, 1, &good), GAT_ERR_ARG, "K = 0");
    expect_refusal(call(100, 5, 0, &good), GAT_ERR_ARG, "E = 0");
    expect_refusal(call(100, 5, 102, &good), GAT_ERR_ARG, "an epoch beyond B");
    expect_refusal(call(100, 4097, 1, &good), GAT_ERR_RANGE, "K range");
    expect_refusal(call((1 << 20) + 1, 5, 1, &good), GAT_ERR_RANGE, "B range");
    gat_obs_config c = good;
    c.struct_size += 8;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_ARG, "struct_size");
    c = good, c.format = 7;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_ARG, "format");
    c = good, c.rx_mode = -1;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_ARG, "rx_mode");
    c = good, c.epoch_stride = 0;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_ARG, "stride");
    c = good, c.epoch_first = -1;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_ARG, "first");
    c = good, c.edge_margin = std::nan("");
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_ARG, "margin");
    c = good, c.travel_ms = 1001;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_RANGE, "travel");
    c = good, c.rx_mode = GAT_OBS_RX_GIVEN, c.rx0_frac = 1e-3;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_RANGE, "rx0_frac");
    c = good, c.code_freq_nominal_hz = 1.0e6;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_RANGE, "code period");
    c = good, c.sampling_freq_hz = 2.5;
    expect_refusal(call(100, 5, 1, &c), GAT_ERR_RANGE, "fs");
}

// walks a plan as the sum and the epoch kernels do
void walk(const ObsPlan &p, bool cells)
{
    const ObsRule &o = p.rule;
    CHECK(p.rows * p.lanes == kObsThreads && p.rows * p.run == kObsChunk && p.lanes >= p.group && (p.lanes & (p.lanes - 1)) == 0, "geometry");
    CHECK((long long)p.groups * p.group >= o.K && (long long)(p.groups - 1) * p.group < o.K, "groups");
    CHECK((long long)p.chunks * kObsChunk >= o.B && (long long)(p.chunks - 1) * kObsChunk < o.B, "chunks");
    CHECK(p.chunk_groups == (long long)p.chunks * p.groups && p.chan_groups * kObsChanWaves >= o.K, "workgroups");
    const size_t cellsz = (size_t)p.chunks * (size_t)o.K;
    CHECK(p.off_totals % 16 == 0 && p.off_bad % 16 == 0 && p.off_runs % 16 == 0 && p.off_chan % 16 == 0 && p.off_anchor % 16 == 0, "alignment");
    CHECK(p.off_totals + cellsz * sizeof(ObsSum) <= p.off_bad && p.off_bad + cellsz * 4 <= p.off_runs &&
              p.off_runs + (size_t)p.chunk_groups * kObsThreads * sizeof(ObsSum) <= p.off_chan && p.off_chan + (size_t)o.K * sizeof(ObsChan) <= p.off_anchor &&
              p.off_anchor + sizeof(ObsAnchor) <= p.bytes && (long long)p.bytes <= kObsMaxScratch,
          "scratch layout");
    for (long long i = 0; i <= o.B; i += 97) {
        const int c = obs_chunk_of(p.chunks, i);
        CHECK(c >= 0 && c < p.chunks && (long long)c * kObsChunk <= i && i - (long long)c * kObsChunk <= kObsChunk, "chunk_of %lld", i);
    }
    if (!cells) return;
    std::vector<unsigned char> covered((size_t)o.B * o.K, 0), written((size_t)o.E * o.K, 0), rx((size_t)o.E, 0);
    for (long long wg = 0; wg < p.chunk_groups; ++wg) {
        int chunk, gi;
        obs_workgroup(p.groups, wg, &chunk, &gi);
        const int kg = obs_group_channels(o.K, p.group, gi);
        CHECK(kg >= 1 && kg <= p.group, "group size");
        for (int t = 0; t < kObsThreads; ++t) {
            int lane, row;
            obs_thread(p.lanes, t, &lane, &row);
            long long i0, i1;
            if (!(lane < kg && obs_run(o.B, p.run, chunk, row, &i0, &i1))) continue;
            const int k = gi * p.group + lane;
            CHECK(k < o.K && i0 >= (long long)chunk * kObsChunk && i1 <= o.B && i1 - i0 <= p.run, "run bounds");
            int e;
            for (long long i = i0; i < i1; ++i) {
                covered[(size_t)i * o.K + k]++;
                if (obs_epoch_at(o, i, &e)) {
                    written[(size_t)e * o.K + k]++;
                    if (k == 0) rx[e]++;
                }
            }
            if (i1 == o.B && obs_epoch_at(o, i1, &e)) {
                written[(size_t)e * o.K + k]++;
                if (k == 0) rx[e]++;
            }
        }
    }
    size_t wrong = 0;
    for (unsigned char v : covered) wrong += v != 1;
    for (unsigned char v : written) wrong += v != 1;
    for (unsigned char v : rx) wrong += v != 1;
    CHECK(wrong == 0, "B %d K %d E %d first %d stride %d: %zu cells not covered exactly once", o.B, o.K, o.E, o.first, o.stride, wrong);
}

int random_plans(int count)
{
    std::mt19937_64 rng(20240917);
    auto pick = [&](long long lo, long long hi) { return (long long)(lo + rng() % (unsigned long long)(hi - lo + 1)); };
    int planned = 0;
    for (int it = 0; it < count; ++it) {
        const int shape = it % 10;
        int B = (int)(shape == 0 ? pick(1, 1 << 20) : shape < 4 ? pick(1, 3 * kObsChunk + 5) : pick(1, 4000));
        int K = (int)(shape == 0 ? pick(1, 4096) : shape < 7 ? pick(1, 70) : pick(1, 600));
        if (it % 17 == 0) B = kObsChunk * (int)pick(1, 4) + (int)pick(-1, 1);
        if (it % 19 == 0) K = kObsThreads + (int)pick(-1, 2);
        gat_obs_config c = config();
        c.epoch_stride = (int)(it % 3 == 0 ? 1 : pick(1, 2 * kObsChunk + 3));
        c.epoch_first = (int)pick(0, B);
        const int most = (B - c.epoch_first) / c.epoch_stride + 1;
        const int E = (int)(it % 2 ? most : pick(1, most));
        ObsPlan p{};
        const Refusal r = obs_plan(call(B, K, E, &c), &p);
        if (r.code != GAT_OK) {
            CHECK(r.code == GAT_ERR_RANGE && (long long)B * K > (1 << 24), "B %d K %d refused: %s", B, K, r.msg);
            continue;
        }
        ++planned;
        gat_obs_plan rep{};
        obs_report(p, &rep);
        CHECK(rep.struct_size == sizeof rep && rep.chunk_blocks == kObsChunk && rep.num_chunks == p.chunks && rep.scratch_bytes == (int64_t)p.bytes, "report");
        walk(p, (long long)B * K <= 3000000);
    }
    return planned;
}

// ---- the twin on exact extents --------------------------------------------------------------------------------------------------------
struct Buffers {
    std::vector<int32_t> tx_ms, rx_ms;
    std::vector<double> tx_frac, rx_frac, carrier_frac, doppler, code_rate;
    std::vector<int64_t> cycles;
    std::vector<gat_obs_channel> channels;
};

void twin_case(int B, int K, int first, int stride, int E, int rx_mode, int format)
{
    gat_obs_config cfg = config();
    cfg.epoch_first = first, cfg.epoch_stride = stride, cfg.rx_mode = rx_mode, cfg.rx0_ms = 604799000, cfg.rx0_frac = 0.0009;
    cfg.format = format, cfg.symbol_blocks = format == GAT_NAV_CNAV ? 10 : 20;
    const int P = format == GAT_NAV_CNAV ? 2 : 1, Pd = cfg.symbol_blocks;
    const double Lc = 1023.0, T = cfg.block_seconds;
    // a history on the heap, exactly [B + 1][K]: channel k starts 3 k ms and a fraction before the frame and runs at its own rates
    std::vector<gat_channel_params> hist((size_t)(B + 1) * K);
    std::vector<int64_t> ms((size_t)(B + 1) * K);
    std::vector<gat_monitor_channel> mon((size_t)K);
    std::vector<gat_nav_channel> nav((size_t)K);
    std::vector<gat_nav_frame> frames((size_t)K * cfg.max_frames);
    std::memset(mon.data(), 0, mon.size() * sizeof mon[0]);
    std::memset(nav.data(), 0, nav.size() * sizeof nav[0]);
    std::memset(frames.data(), 0, frames.size() * sizeof frames[0]);
    const int64_t frame_ms = 604800000 - 6000; // the last frame of the week: tow 0
    for (int k = 0; k < K; ++k) {
        const double rate = 1.023e6 + (k % 2 ? -35.0 : 35.0), fcarr = (k % 2 ? -1.0 : 1.0) * (1000.0 + 37.0 * k);
        const int g = B >= 2 ? (B / 2 + k) % (B + 1) : B;
        // walk from block 0: the transmit time there is chosen so that block g starts 0.2 periods after the frame's first millisecond
        double tau = 0.2 * Lc;
        int64_t m = frame_ms;
        // backwards to block 0
        std::vector<double> taus((size_t)B + 1);
        std::vector<int64_t> mss((size_t)B + 1);
        taus[g] = tau, mss[g] = m;
        for (int b = g - 1; b >= 0; --b) {
            double x = taus[b + 1] - rate * T;
            const double w = std::floor(x / Lc);
            x -= w * Lc;
            taus[b] = x, mss[b] = mss[b + 1] + (int64_t)w;
        }
        for (int b = g; b < B; ++b) {
            double x = taus[b] + rate * T;
            const double w = std::floor(x / Lc);
            x -= w * Lc;
            taus[b + 1] = x, mss[b + 1] = mss[b] + (int64_t)w;
        }
        double phi = 0.25;
        for (int b = 0; b <= B; ++b) {
            gat_channel_params &r = hist[(size_t)b * K + k];
            r.prn = k, r.reserved = 0, r.code_freq_hz = rate, r.carrier_freq_hz = fcarr, r.code_phase_chips = taus[b], r.carrier_phase_cycles = phi;
            ms[(size_t)b * K + k] = obs_mod(mss[b], kObsWeekMs);
            const double y = phi + fcarr * T;
            phi = y - std::floor(y);
        }
        const int symbols = g / Pd;
        mon[k].start = mon[k].symbol_offset = g % Pd, mon[k].num_symbols = (B - g % Pd) / Pd;
        nav[k].symbol_phase = symbols % P, nav[k].frame_offset = symbols / P, nav[k].num_frames = 2, nav[k].tow_steps = 1;
        for (int f = 0; f < 2; ++f) {
            gat_nav_frame &fr = frames[(size_t)k * cfg.max_frames + f];
            fr.status = f == 0 ? 0x1 : (format == GAT_NAV_CNAV ? 0x3 : 0x7ff); // f* = 1: frame 0 failed a check
            fr.tow = f;                                                       // frame 1 carries tow 1: frame 0 began at (1 - 1 - 1) mod 100800
        }
    }
    Buffers full;
    const size_t EK = (size_t)E * K;
    for (int variant = -1; variant < 18; ++variant) {
        // -1: every output; 0 .. 8: that output alone; 9 .. 17: all but that output
        auto given = [&](int i) { return variant < 0 || (variant < 9 ? i == variant : i != variant - 9); };
        Buffers b;
        if (given(0)) b.tx_ms.assign(EK, 77);
        if (given(1)) b.tx_frac.assign(EK, 77.0);
        if (given(2)) b.rx_ms.assign((size_t)E, 77);
        if (given(3)) b.rx_frac.assign((size_t)E, 77.0);
        if (given(4)) b.cycles.assign(EK, 77);
        if (given(5)) b.carrier_frac.assign(EK, 77.0);
        if (given(6)) b.doppler.assign(EK, 77.0);
        if (given(7)) b.code_rate.assign(EK, 77.0);
        if (given(8)) b.channels.resize((size_t)K);
        ObsOut o{};
        o.tx_ms = given(0) ? b.tx_ms.data() : nullptr, o.tx_frac = given(1) ? b.tx_frac.data() : nullptr;
        o.rx_ms = given(2) ? b.rx_ms.data() : nullptr, o.rx_frac = given(3) ? b.rx_frac.data() : nullptr;
        o.carrier_cycles = given(4) ? b.cycles.data() : nullptr, o.carrier_frac = given(5) ? b.carrier_frac.data() : nullptr;
        o.doppler_hz = given(6) ? b.doppler.data() : nullptr, o.code_rate_hz = given(7) ? b.code_rate.data() : nullptr;
        o.channels = given(8) ? b.channels.data() : nullptr;
        ObsPlan p{};
        const Refusal r = obs_plan(ObsCall{hist.data(), mon.data(), nav.data(), frames.data(), B, K, E, &cfg, o}, &p);
        CHECK(r.code == GAT_OK, "twin case refused: %s", r.msg ? r.msg : "");
        if (r.code != GAT_OK) return;
        obs_host_run(p, hist.data(), mon.data(), nav.data(), frames.data(), o);
        if (variant < 0) {
            full = b;
            for (int e = 0; e < E; ++e)
                for (int k = 0; k < K; ++k) {
                    const size_t at = (size_t)e * K + k, hb = ((size_t)first + (size_t)e * stride) * K + k;
                    CHECK(b.tx_ms[at] == ms[hb], "B %d K %d e %d k %d: tx_ms %d, truth %lld (status %d)", B, K, e, k, b.tx_ms[at], (long long)ms[hb],
                          b.channels[k].status);
                    CHECK(b.tx_frac[at] == hist[hb].code_phase_chips / 1.023e6 && b.tx_frac[at] < 1e-3, "tx_frac");
                    CHECK(b.code_rate[at] == hist[hb].code_freq_hz && b.carrier_frac[at] == hist[hb].carrier_phase_cycles, "carrier outputs");
                }
            for (int k = 0; k < K; ++k)
                CHECK(b.channels[k].status == 0 && b.channels[k].tow_frame == 1 && b.channels[k].frame0_ms == 604794000, "channel %d status %d", k,
                      b.channels[k].status);
            for (int e = 0; e < E; ++e) CHECK(b.rx_ms[e] >= 0 && b.rx_ms[e] < 604800000 && b.rx_frac[e] >= 0.0 && b.rx_frac[e] < 1e-3, "rx");
        } else {
            CHECK(!given(0) || b.tx_ms == full.tx_ms, "subset tx_ms");
            CHECK(!given(1) || b.tx_frac == full.tx_frac, "subset tx_frac");
            CHECK(!given(2) || b.rx_ms == full.rx_ms, "subset rx_ms");
            CHECK(!given(3) || b.rx_frac == full.rx_frac, "subset rx_frac");
            CHECK(!given(4) || b.cycles == full.cycles, "subset cycles");
            CHECK(!given(5) || b.carrier_frac == full.carrier_frac, "subset carrier_frac");
            CHECK(!given(6) || b.doppler == full.doppler, "subset doppler");
            CHECK(!given(7) || b.code_rate == full.code_rate, "subset code_rate");
            CHECK(!given(8) || std::memcmp(b.channels.data(), full.channels.data(), (size_t)K * sizeof(gat_obs_channel)) == 0, "subset channels");
        }
    }
}

} // namespace

int main()
{
    refusals();
    const int planned = random_plans(3000);
    twin_case(1, 1, 0, 1, 2, GAT_OBS_RX_FROM_TX, GAT_NAV_LNAV);
    twin_case(2, 3, 2, 1, 1, GAT_OBS_RX_GIVEN, GAT_NAV_LNAV);
    twin_case(kObsChunk + 1, 5, 0, 1, kObsChunk + 2, GAT_OBS_RX_FROM_TX, GAT_NAV_LNAV);
    twin_case(2 * kObsChunk + 3, 65, 7, 300, 2, GAT_OBS_RX_GIVEN, GAT_NAV_CNAV);
    twin_case(777, 12, 17, 20, 39, GAT_OBS_RX_FROM_TX, GAT_NAV_CNAV);
    std::printf("planned %d calls, ran the twin on 5 cases: %d failures\n", planned, failures);
    return failures ? 1 : 0;
}
