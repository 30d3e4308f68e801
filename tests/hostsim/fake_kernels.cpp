// fake_kernels.cpp -- stand-ins for libgat's kernel launchers (the functions gat_kernels.hip, gat_dc_f*.hip, gat_mfma*.hip,
// gat_resident_f*.hip, gat_acq.hip and gat_array.hip define): nothing is computed.  Instead every launch of the correlator's kernels is
// checked against what they ASSUME about their arguments (tests/corr_launch_contract.h, shared with tests/corrplan): the planner's
// contract, over thousands of random shapes, under ASan / UBSan on the CPU.  A launch of the resident kernel starts a host thread that
// plays the device's side of the doorbell protocol (gat_resident.h), so that gat_resident_*'s host side -- ring, wait, second stage,
// restart after the kernel has left -- runs for real.  Test infrastructure only.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "gat_acq_kernels.h"
#include "gat_array_kernels.h"
#include "gat_ctx.h"
#include "../corr_launch_contract.h"
#include "hostsim.h"

namespace gat {

using hostsim::counters;

// what REQUIRE (corr_launch_contract.h) calls, here and in the contract's checks
__attribute__((format(printf, 2, 3))) static void broken(const char *cond, const char *fmt, ...)
{
    ++counters.violations;
    std::fprintf(stderr, "planner invariant broken: %s -- ", cond);
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "\n");
}

hipError_t launch_dc(const DcArgs &a, const DcLaunch &cfg, hipStream_t)
{
    ++counters.dc_launches;
    check_dc(a, cfg, false, broken);
    for (int l = 0; l < cfg.taps && l < kMaxTapsPerLaunch; ++l) hostsim::tap_cover.main.emplace_back(a.tap_index[l], a.shifts[l]);
    return hipSuccess;
}
hipError_t launch_finalize(const float *partial, float *out_re, float *out_im, int splits, int elems, long long groups, hipStream_t, unsigned *done, unsigned *flag, unsigned seq)
{
    ++counters.finalize_launches;
    REQUIRE(partial && out_re && out_im && splits >= 1 && elems >= 2 && elems % 2 == 0 && groups >= 1, "finalize: %d splits x %d elems x %lld groups", splits, elems, groups);
    REQUIRE((done == nullptr) == (seq == 0) || flag != nullptr, "finalize: completion flag half set");
    return hipSuccess;
}
hipError_t launch_dc_tail(const DcTailArgs &a, hipStream_t)
{
    ++counters.tail_launches;
    hostsim::tap_cover.tail.emplace_back(a.shifts, a.shifts + std::min(std::max(a.L, 0), (int)GAT_MAX_TAPS));
    REQUIRE(a.n_vec < a.N && a.N - a.n_vec < 8 && a.out_re && a.out_im, "tail: n_vec %d of %lld", a.n_vec, a.N);
    return hipSuccess;
}
hipError_t launch_mfma(const MfArgs &a, int nct, unsigned grid, unsigned lds_bytes, hipStream_t)
{
    ++counters.mfma_launches;
    check_mfma(a, nct, grid, lds_bytes, broken);
    for (int l = 0; l < a.L && l < kMfmaMaxTaps; ++l) hostsim::tap_cover.main.emplace_back(a.tap_index[l], a.shifts[l]);
    return hipSuccess;
}
hipError_t launch_mfma_bf16(const MfArgs &a, int rt, int nct, int fmt, unsigned grid, unsigned lds_bytes, hipStream_t)
{
    ++counters.mfma_launches;
    check_mfma_bf16(a, rt, nct, fmt, grid, lds_bytes, broken);
    for (int l = 0; l < a.L && l < kMfmaMaxTaps; ++l) hostsim::tap_cover.main.emplace_back(a.tap_index[l], a.shifts[l]);
    return hipSuccess;
}

hipError_t launch_gen_code_replica(float *, long long, const int8_t *, int, double, double, double, long long, bool, hipStream_t) { ++counters.other_launches; return hipSuccess; }
hipError_t launch_gen_code_replica_texaddr(float *, long long, const int8_t *, int, double, double, double, long long, int coord_bits, int texel_bits, hipStream_t)
{
    ++counters.other_launches;
    REQUIRE(coord_bits >= 0 && coord_bits <= 32 && texel_bits >= -1 && texel_bits <= 24, "texture addressing study: %d / %d bits", coord_bits, texel_bits);
    return hipSuccess;
}
hipError_t launch_read_stream(const void *dev, size_t bytes, int variant, int num_cus, float *sink, hipStream_t)
{
    ++counters.other_launches;
    REQUIRE(dev && sink && bytes >= 16 && bytes % 16 == 0 && variant >= 0 && variant < 16 && num_cus > 0, "read stream: %zu bytes, variant %d", bytes, variant);
    return hipSuccess;
}
hipError_t launch_gen_code_replica_multi(float *, long long, long long, int, const gat_channel_params *, const int8_t *, int, int, int, double, long long, hipStream_t) { ++counters.other_launches; return hipSuccess; }
hipError_t launch_accumulate_debug(const float *, const float *, long long, int, long long, const gat_channel_params &, const int8_t *, int, double, int, const int *, float *, float *, float *, float *, float *, float *, hipStream_t) { ++counters.other_launches; return hipSuccess; }
hipError_t launch_gen_signal(void *, void *, int, long long, int, long long, long long, int, int, const gat_channel_params *, const int8_t *, int, int, int, double, float, const float *, float, unsigned long long, hipStream_t) { ++counters.other_launches; return hipSuccess; }
hipError_t launch_reduce_stage1(const float *, const float *, long long, int, int, float *, hipStream_t) { ++counters.other_launches; return hipSuccess; }
hipError_t launch_tracking_update(const float *, const float *, int, int, const gat_loop_config &, gat_loop_state *, const gat_channel_params *cur, gat_channel_params *next, hipStream_t)
{
    ++counters.other_launches;
    REQUIRE(cur != nullptr && next != nullptr && cur != next, "tracking update: parameter ping-pong");
    return hipSuccess;
}

// ---- the acquisition search (gat_acq.hip) ---------------------------------------------------------------------------------
// Each launch is checked against what acq_grid_kernel / acq_sum_groups_kernel / acq_stats_kernel assume, and every byte a
// kernel would read or write is touched, so that ASan reports a wrong offset in gat_acquire's scratch carve-up.
static size_t acq_allowed_lds = 0;            // what acq_grid_allow_lds granted last
static const float *acq_last_grid_out = nullptr; // the grid launch's `out`, for the group sum and statistics that follow
static long long acq_last_cells = 0;
static int acq_last_G = 0;

hipError_t acq_grid_allow_lds(int s)
{
    const size_t lds = acq_grid_lds_bytes(s);
    REQUIRE(s >= 1 && s <= kAcqMaxCodeStep && lds <= 160 * 1024, "acq: LDS %zu bytes for code step %d", lds, s);
    acq_allowed_lds = lds;
    return hipSuccess;
}

hipError_t launch_acq_grid(const AcqArgs &a, int fmt, hipStream_t)
{
    ++counters.acq_grid_launches;
    if (a.G > 1) ++counters.acq_split_launches;
    const long long jt = (a.J + kAcqCodeTile - 1) / kAcqCodeTile, dt = (a.D + kAcqDopTile - 1) / kAcqDopTile;
    const long long z = (long long)a.P * a.G, cells = (long long)a.P * a.D * a.J, units = (long long)a.M * a.B;
    REQUIRE(fmt >= GAT_LAYOUT_PLANAR && fmt <= GAT_LAYOUT_INTERLEAVED_I8 && (fmt == GAT_LAYOUT_PLANAR) == (a.im != nullptr) && a.re,
            "acq: layout %d", fmt);
    REQUIRE(a.P >= 1 && a.D >= 1 && a.J >= 1 && z <= 65535 && jt <= 0x7fffffff && dt <= 65535, "acq: grid %lld x %lld x %lld", jt, dt, z);
    REQUIRE(a.G >= 1 && a.G <= units, "acq: %d groups for %lld units", a.G, units);
    REQUIRE(a.s >= 1 && a.s <= kAcqMaxCodeStep && acq_grid_lds_bytes(a.s) <= acq_allowed_lds && acq_allowed_lds <= 160 * 1024,
            "acq: code step %d, LDS %zu of %zu allowed", a.s, acq_grid_lds_bytes(a.s), acq_allowed_lds);
    REQUIRE(a.N >= 1 && a.M >= 1 && a.B >= 1 && (a.M == 1 || a.ant_stride >= 1) && (a.B == 1 || a.block_stride >= 1), "acq: signal %lld x %d x %d", a.N, a.M, a.B);
    // the replica window: sample index x = n0 + first_shift + s j0 + e, e < kAcqChunk + s (kAcqCodeTile - 1), as the kernel
    // evaluates it (an int), within what chip_index evaluates exactly for any tau in [0, Lc) (code_span_bad)
    const long long last_n0 = (a.N - 1) / kAcqChunk * kAcqChunk, rep_len = kAcqChunk + (long long)a.s * (kAcqCodeTile - 1);
    const long long x_lo = a.first_shift, x_hi = last_n0 + a.first_shift + (long long)a.s * (jt - 1) * kAcqCodeTile + rep_len - 1;
    const double reach = (double)std::max(std::llabs(x_lo), std::llabs(x_hi));
    REQUIRE(x_lo > INT32_MIN && x_hi < INT32_MAX, "acq: window index %lld .. %lld", x_lo, x_hi);
    REQUIRE(!code_span_bad(a.ratio, (double)a.Lc, reach, a.Lc), "acq: code span for ratio %g over %g samples", a.ratio, reach);
    REQUIRE(a.ratio > 0.0 && std::isfinite(a.fs) && a.fs > 0.0, "acq: ratio %g fs %g", a.ratio, a.fs);
    // the PRNs' code rows, the signal's first and last sample of every (antenna, block) unit, the output slices
    volatile long sink = 0;
    for (int p = 0; p < a.P; ++p) {
        REQUIRE(a.prns[p] >= 0, "acq: prn %d", a.prns[p]);
        sink += a.codes[(size_t)a.prns[p] * a.code_row_stride] + a.codes[(size_t)a.prns[p] * a.code_row_stride + a.Lc - 1];
    }
    const size_t bytes = fmt == GAT_LAYOUT_PLANAR ? 4 : fmt == GAT_LAYOUT_INTERLEAVED ? 8 : fmt == GAT_LAYOUT_INTERLEAVED_I16 ? 4 : 2;
    for (long long u = 0; u < units; ++u) {
        const long long m = u % a.M, b = u / a.M;
        for (const long long n : {0ll, a.N - 1}) {
            const size_t e = (size_t)(b * a.block_stride + m * a.ant_stride + n);
            if (fmt == GAT_LAYOUT_PLANAR) {
                sink += static_cast<const unsigned char *>(a.re)[e * bytes + bytes - 1] + static_cast<const unsigned char *>(a.im)[e * bytes];
            } else {
                sink += static_cast<const unsigned char *>(a.re)[e * bytes] + static_cast<const unsigned char *>(a.re)[e * bytes + bytes - 1];
            }
        }
    }
    (void)sink;
    const auto *o0 = reinterpret_cast<const unsigned char *>(a.out), *o1 = o0 + (size_t)a.G * cells * sizeof(float);
    const auto *q0 = reinterpret_cast<const unsigned char *>(a.prns), *q1 = q0 + (size_t)a.P * sizeof(int);
    REQUIRE(o1 <= q0 || q1 <= o0, "acq: the grid's output overlaps the PRN list");
    std::memset(a.out, 0, (size_t)a.G * cells * sizeof(float));
    acq_last_grid_out = a.out;
    acq_last_cells = cells;
    acq_last_G = a.G;
    return hipSuccess;
}

hipError_t launch_acq_sum_groups(const float *part, float *power, long long cells, int G, hipStream_t)
{
    ++counters.other_launches;
    REQUIRE(G > 1 && G == acq_last_G && part == acq_last_grid_out && cells == acq_last_cells, "acq: group sum of %d slices", G);
    REQUIRE(power + cells <= part || part + (size_t)G * cells <= power, "acq: the group sum's output overlaps its slices");
    volatile float sink = part[0] + part[(size_t)G * cells - 1];
    (void)sink;
    std::memset(power, 0, (size_t)cells * sizeof(float));
    acq_last_grid_out = power;
    return hipSuccess;
}

hipError_t launch_acq_stats(const float *power, int P, int D, int J, const gat_acq_config &cfg, double fs, long long N,
                            const int *prns, gat_acq_result *res, hipStream_t)
{
    ++counters.other_launches;
    REQUIRE(power == acq_last_grid_out && (long long)P * D * J == acq_last_cells, "acq: statistics of a grid the search did not write");
    REQUIRE(cfg.code_length >= 1 && cfg.num_doppler_bins == D && cfg.num_code_bins == J && N >= 1 && fs > 0.0, "acq: statistics config");
    const auto *r0 = reinterpret_cast<const unsigned char *>(res), *r1 = r0 + (size_t)P * sizeof(gat_acq_result);
    const auto *g0 = reinterpret_cast<const unsigned char *>(power), *g1 = g0 + (size_t)P * D * J * sizeof(float);
    const auto *q0 = reinterpret_cast<const unsigned char *>(prns), *q1 = q0 + (size_t)P * sizeof(int);
    REQUIRE((r1 <= g0 || g1 <= r0) && (r1 <= q0 || q1 <= r0), "acq: the results overlap the grid or the PRN list");
    volatile float sink = power[0] + power[(size_t)P * D * J - 1];
    for (int p = 0; p < P; ++p) {
        sink = sink + (float)prns[p];
        std::memset(&res[p], 0, sizeof(gat_acq_result));
        res[p].prn = prns[p];
    }
    (void)sink;
    return hipSuccess;
}

// ---- the antenna-array path (gat_array.hip) -------------------------------------------------------------------------------
// The covariance stand-ins check what cov_small_kernel / cov_tiled_kernel assume about CovArgs, walk the (estimate, workgroup,
// unit) decomposition as CovArgs documents it, touch the first and last byte every unit reads of every antenna and plane, write
// the whole slice of `partial` every workgroup owns, and count every (block, sample) in hostsim::cov_cover.
static const float *cov_last_partial = nullptr; // the covariance launch's slices, for the finishing launch that follows
static int cov_last_M = 0, cov_last_E = 0, cov_last_G = 0;

static void cov_walk(const CovArgs &a, int fmt, const char *tag)
{
    const size_t sb = (size_t)layout_sample_bytes(fmt);
    const bool planar = fmt == GAT_LAYOUT_PLANAR;
    REQUIRE(fmt >= GAT_LAYOUT_PLANAR && fmt <= GAT_LAYOUT_INTERLEAVED_I8 && a.re && planar == (a.im != nullptr), "%s: layout %d", tag, fmt);
    REQUIRE(a.M >= 1 && a.M <= GAT_MAX_ARRAY_ANTS && a.N >= 1 && a.B >= 1 && a.bpe >= 1 && a.E == (a.B + a.bpe - 1) / a.bpe, "%s: M %d N %lld B %d bpe %d E %d",
            tag, a.M, a.N, a.B, a.bpe, a.E);
    REQUIRE(a.splits >= 1 && a.seg_len >= 1 && (long long)a.splits * a.seg_len >= a.N && (long long)(a.splits - 1) * a.seg_len < a.N,
            "%s: %d segments of %lld for N %lld (an empty segment would add the block's tail again)", tag, a.splits, a.seg_len, a.N);
    REQUIRE(a.G >= 1 && (long long)a.G * a.E <= 0x7fffffffll, "%s: grid of %d x %d workgroups", tag, a.G, a.E);
    REQUIRE((a.M == 1 || a.ant_stride >= 1) && (a.B == 1 || a.block_stride >= 1) && a.partial != nullptr, "%s: strides %lld / %lld", tag, a.ant_stride,
            a.block_stride);
    if (a.splits > 1) ++counters.cov_split_launches;
    if ((long long)std::min(a.bpe, a.B) * a.splits > a.G) ++counters.cov_multi_unit_launches;
    auto &cv = hostsim::cov_cover;
    // block 0 of this launch within the call (the entry point offsets the planes by whole blocks from one batch to the next)
    const long long byte_off = static_cast<const char *>(a.re) - static_cast<const char *>(cv.re);
    const long long blk_bytes = cv.block_stride * (long long)sb;
    const long long first_block = blk_bytes > 0 ? byte_off / blk_bytes : 0;
    REQUIRE(byte_off >= 0 && (blk_bytes > 0 ? byte_off % blk_bytes == 0 : byte_off == 0) && a.N == cv.N && a.block_stride == cv.block_stride &&
                first_block + a.B <= cv.B,
            "%s: launch of %d blocks %lld bytes into a call of %d blocks", tag, a.B, byte_off, cv.B);
    if (counters.violations) return; // (do not walk a decomposition that is already known to be wrong)
    const size_t slice = (size_t)2 * a.M * a.M;
    volatile long sink = 0;
    for (int e = 0; e < a.E; ++e) {
        const int b0 = e * a.bpe, nb = std::min(a.bpe, a.B - b0);
        const long long units = (long long)nb * a.splits;
        for (int g = 0; g < a.G; ++g) {
            for (long long u = g; u < units; u += a.G) {
                const int b = b0 + (int)(u / a.splits);
                const long long n0 = (u % a.splits) * a.seg_len, n1 = std::min(n0 + a.seg_len, a.N);
                for (int m = 0; m < a.M; ++m) {
                    const size_t s0 = (size_t)b * (size_t)a.block_stride + (size_t)m * (size_t)a.ant_stride;
                    const unsigned char *r = static_cast<const unsigned char *>(a.re) + s0 * sb;
                    sink = sink + r[(size_t)n0 * sb] + r[(size_t)n1 * sb - 1];
                    if (planar) {
                        const unsigned char *q = static_cast<const unsigned char *>(a.im) + s0 * sb;
                        sink = sink + q[(size_t)n0 * sb] + q[(size_t)n1 * sb - 1];
                    }
                }
                unsigned char *row = cv.seen.data() + (size_t)(first_block + b) * (size_t)a.N;
                for (long long n = n0; n < n1; ++n)
                    if (row[n] < 255) ++row[n];
            }
            std::memset(a.partial + ((size_t)e * a.G + g) * slice, 0, slice * sizeof(float));
        }
    }
    (void)sink;
    cov_last_partial = a.partial;
    cov_last_M = a.M, cov_last_E = a.E, cov_last_G = a.G;
}

hipError_t launch_cov_small(const CovArgs &a, int fmt, hipStream_t)
{
    ++counters.cov_small_launches;
    const long long vs = layout_vec_samples(fmt);
    const size_t sb = (size_t)layout_sample_bytes(fmt);
    REQUIRE(a.M >= 1 && a.M <= kCovSmallMaxAnts, "streaming covariance: %d antennas", a.M);
    REQUIRE(a.seg_len % vs == 0, "streaming covariance: segments of %lld samples, loads of %lld", a.seg_len, vs);
    bool aligned = true; // every (block, antenna) start, in each plane
    for (int b = 0; b < a.B && aligned; ++b)
        for (int m = 0; m < a.M && aligned; ++m) {
            const size_t off = ((size_t)b * (size_t)a.block_stride + (size_t)m * (size_t)a.ant_stride) * sb;
            aligned = ((reinterpret_cast<uintptr_t>(a.re) + off) & 15u) == 0 && (!a.im || ((reinterpret_cast<uintptr_t>(a.im) + off) & 15u) == 0);
        }
    REQUIRE(aligned, "streaming covariance: a block of an antenna starts off a 16-byte boundary (strides %lld / %lld)", a.ant_stride, a.block_stride);
    cov_walk(a, fmt, "streaming covariance");
    return hipSuccess;
}

hipError_t launch_cov_tiled(const CovArgs &a, int fmt, hipStream_t)
{
    ++counters.cov_tiled_launches;
    const CovTileGeom geo = cov_tile_geom(std::max(1, std::min(a.M, (int)GAT_MAX_ARRAY_ANTS)));
    REQUIRE(geo.lds_bytes <= 64 * 1024 && (size_t)geo.chunk * geo.row * 8 <= geo.lds_bytes && (size_t)kCovTileThreads * 16 * sizeof(float) <= geo.lds_bytes,
            "tiled covariance: %zu bytes of LDS for M %d", geo.lds_bytes, a.M);
    REQUIRE(geo.phases >= 1 && geo.per_phase >= 1 && geo.tiles * geo.phases <= kCovTileThreads && geo.chunk == geo.phases * geo.per_phase &&
                geo.row >= geo.nt * kCovTile && geo.nt * kCovTile >= a.M && geo.row % 2 == 0,
            "tiled covariance: geometry %d tiles x %d phases, rows of %d for M %d", geo.tiles, geo.phases, geo.row, a.M);
    cov_walk(a, fmt, "tiled covariance");
    return hipSuccess;
}

hipError_t launch_cov_finish(const float *partial, int M, int E, int G, float *cov_re, float *cov_im, hipStream_t)
{
    ++counters.cov_finish_launches;
    REQUIRE(partial && partial == cov_last_partial && M == cov_last_M && E == cov_last_E && G == cov_last_G && cov_re && cov_im,
            "covariance finish: %d x %d slices of M %d after a launch of %d x %d of M %d", E, G, M, cov_last_E, cov_last_G, cov_last_M);
    const size_t slice = (size_t)2 * M * M;
    volatile float sink = 0.f;
    for (size_t s = 0; s < (size_t)E * G; ++s) sink = sink + partial[s * slice] + partial[s * slice + slice - 1];
    (void)sink;
    std::memset(cov_re, 0, (size_t)E * M * M * sizeof(float));
    std::memset(cov_im, 0, (size_t)E * M * M * sizeof(float));
    return hipSuccess;
}

// The launcher's signature carries no LDS request (gat_array.hip derives it from M and the mode), so what can be checked here
// is only that the entry point asked for the larger LDS limit before it launched, and that M is within what that limit holds.
static bool weights_lds_allowed = false;
hipError_t array_weights_allow_lds()
{
    weights_lds_allowed = true;
    return hipSuccess;
}

hipError_t launch_array_weights(const float *cov_re, const float *cov_im, int M, const double *steer_re, const double *steer_im, int K, int mode,
                                double loading, double *scratch, double *w_re, double *w_im, hipStream_t)
{
    ++counters.array_weight_launches;
    const bool conv = mode == GAT_BF_CONVENTIONAL, pinv = mode == GAT_BF_POWER_INVERSION;
    REQUIRE(M >= 1 && M <= GAT_MAX_ARRAY_ANTS && K >= 1 && K <= 65535 && (conv || pinv || mode == GAT_BF_MVDR) && w_re && w_im && loading >= 0.0,
            "weights: M %d K %d mode %d", M, K, mode);
    REQUIRE(conv || (cov_re && cov_im && scratch), "weights: mode %d without a covariance or scratch", mode);
    REQUIRE(pinv || (steer_re && steer_im), "weights: mode %d without steering vectors", mode);
    REQUIRE(weights_lds_allowed, "weights: launched before array_weights_allow_lds (64 antennas need more than 64 KB of LDS)");
    if (counters.violations) return hipSuccess;
    volatile double sink = 0.0;
    if (!conv) {
        sink = sink + cov_re[0] + cov_re[(size_t)M * M - 1] + cov_im[0] + cov_im[(size_t)M * M - 1];
        std::memset(scratch, 0, (size_t)2 * M * M * sizeof(double) + sizeof(int)); // l_re | l_im | ok
    }
    if (!pinv) sink = sink + steer_re[0] + steer_re[(size_t)K * M - 1] + steer_im[0] + steer_im[(size_t)K * M - 1];
    (void)sink;
    std::memset(w_re, 0, (size_t)K * M * sizeof(double));
    std::memset(w_im, 0, (size_t)K * M * sizeof(double));
    return hipSuccess;
}

hipError_t launch_beamform(const float *acc_re, const float *acc_im, long long rows, int K, int L, int M, const double *w_re, const double *w_im,
                           float *out_re, float *out_im, hipStream_t)
{
    ++counters.beamform_launches;
    REQUIRE(acc_re && acc_im && w_re && w_im && out_re && out_im && K >= 1 && L >= 1 && M >= 1 && rows >= 1 && rows % ((long long)K * L) == 0 &&
                (rows + 255) / 256 <= 0x7fffffffll,
            "beamform: %lld rows for K %d L %d M %d", rows, K, L, M);
    if (counters.violations) return hipSuccess;
    volatile double sink = acc_re[0] + acc_re[(size_t)rows * M - 1] + acc_im[0] + acc_im[(size_t)rows * M - 1];
    sink = sink + w_re[0] + w_re[(size_t)K * M - 1] + w_im[0] + w_im[(size_t)K * M - 1];
    (void)sink;
    std::memset(out_re, 0, (size_t)rows * sizeof(float));
    std::memset(out_im, 0, (size_t)rows * sizeof(float));
    return hipSuccess;
}

hipError_t launch_tracking_update_weighted(const float *acc_re, const float *acc_im, int K, int M, const gat_loop_config &cfg, gat_loop_state *state,
                                           const gat_channel_params *cur, gat_channel_params *next, const double *w_re, const double *w_im,
                                           hipStream_t)
{
    ++counters.weighted_update_launches;
    const int L = cfg.num_taps;
    REQUIRE(acc_re && acc_im && state && cur && next && cur != next && w_re && w_im && K >= 1 && M >= 1, "weighted update: K %d M %d", K, M);
    REQUIRE(L >= 1 && L <= GAT_MAX_TAPS && cfg.early_index >= 0 && cfg.early_index < L && cfg.prompt_index >= 0 && cfg.prompt_index < L &&
                cfg.late_index >= 0 && cfg.late_index < L,
            "weighted update: taps %d / %d / %d of %d", cfg.early_index, cfg.prompt_index, cfg.late_index, L);
    if (counters.violations) return hipSuccess;
    const size_t n = (size_t)K * L * M;
    volatile double sink = acc_re[0] + acc_re[n - 1] + acc_im[0] + acc_im[n - 1] + w_re[0] + w_re[(size_t)K * M - 1] + w_im[0] + w_im[(size_t)K * M - 1];
    sink = sink + state[0].pll_acc1 + state[K - 1].pll_acc1 + cur[0].code_freq_hz + cur[K - 1].code_freq_hz;
    (void)sink;
    for (int k = 0; k < K; ++k) next[k] = cur[k];
    return hipSuccess;
}

// ---- the resident kernel, played by a host thread -------------------------------------------------------------------------
} // namespace gat
namespace hostsim {
float resident_value(unsigned slot, int o) { return (float)(slot * 64u + (unsigned)o) + 0.5f; }
} // namespace hostsim
namespace gat {

static void resident_device(DcArgs a, DcLaunch cfg, ResidentArgs r)
{
    using clk = std::chrono::steady_clock;
    const int nval = 2 * cfg.ant_tile * cfg.taps, lw = (nval + kResLinePayload - 1) / kResLinePayload;
    auto ld = [](const unsigned *p) { return __atomic_load_n(p, __ATOMIC_ACQUIRE); };
    unsigned last = r.start_seq, calls = 0, why = kResidentRuns;
    const auto t_start = clk::now();
    auto t_last = t_start;
    auto ticks = [](clk::duration d) { return std::chrono::duration_cast<std::chrono::nanoseconds>(d).count() / 10; }; // 100 MHz
    unsigned poll = 0;
    for (;;) {
        const unsigned *bell = r.host_bell + (size_t)(poll++ % (unsigned)r.bell_copies) * kResMaxChannels * kBellDwords; // (a copy per workgroup: all must ring)
        const unsigned seq = ld(bell);
        if (seq == kBellQuit) { why = kResidentQuit; break; }
        if (seq != last) {
            bool ok = true;
            for (int k = 0; k < a.K && ok; ++k) {
                const unsigned *ln = bell + k * kBellDwords;
                unsigned x = 0, w[kBellDwords];
                for (int i = 0; i < kBellDwords; ++i) w[i] = ld(ln + i);
                for (int i = 0; i < 14; ++i) x ^= w[i];
                ok = w[0] == seq && w[15] == seq && w[14] == x;
                if (ok) { // the record the host rang: what the kernel would read
                    gat_channel_params p;
                    std::memcpy(&p, &w[2], sizeof p);
                    long long off;
                    std::memcpy(&off, &w[12], sizeof off);
                    if (!(p.prn >= 0 && p.prn < a.num_prns && off >= 0 && p.reserved == 0)) {
                        ++counters.violations;
                        std::fprintf(stderr, "resident: bad record in a validated ring (prn %d, offset %lld)\n", p.prn, off);
                    }
                }
            }
            if (ok) {
                // every working workgroup posts its lines (here: one after the other, last line of the last slot last)
                for (unsigned slot = 0; slot < a.total_wgs; ++slot)
                    for (int j = 0; j < lw; ++j) {
                        unsigned *ln = r.host_lines + ((size_t)slot * lw + j) * 16, x = seq;
                        for (int i = 0; i < kResLinePayload; ++i) {
                            const int o = j * kResLinePayload + i;
                            const float v = o < nval ? hostsim::resident_value(slot, o) : 0.f;
                            unsigned u;
                            std::memcpy(&u, &v, 4);
                            x ^= u;
                            __atomic_store_n(ln + i, u, __ATOMIC_RELAXED);
                        }
                        __atomic_store_n(ln + 14, x, __ATOMIC_RELAXED);
                        __atomic_store_n(ln + 15, seq, __ATOMIC_RELEASE);
                    }
                last = seq;
                ++calls;
                ++counters.resident_calls;
                t_last = clk::now();
                continue;
            }
        }
        const auto now = clk::now();
        if (calls >= r.max_calls) { why = kResidentCalls; break; }
        if (ticks(now - t_last) > r.idle_ticks) { why = kResidentIdle; break; }
        if (ticks(now - t_start) > r.life_ticks) { why = kResidentLife; break; }
    }
    r.host_state[1] = calls;
    __atomic_store_n(r.host_state, why, __ATOMIC_RELEASE);
}

// what one "compute unit" of the simulated device holds of a resident instance: two workgroups by the occupancy API's word
// (the library takes one off every answer above one)
hipError_t dc_resident_blocks_per_cu(const DcLaunch &cfg, int *blocks_per_cu)
{
    REQUIRE(blocks_per_cu != nullptr && cfg.format >= GAT_LAYOUT_PLANAR && cfg.format <= GAT_LAYOUT_INTERLEAVED_I8 && dc_resident_instance(cfg.ant_tile, cfg.taps), "resident occupancy query: instance");
    *blocks_per_cu = 2;
    return hipSuccess;
}

hipError_t launch_dc_resident(const DcArgs &a, const DcLaunch &cfg, const ResidentArgs &r, hipStream_t s)
{
    ++counters.resident_starts;
    check_dc(a, cfg, true, broken);
    REQUIRE((r.bell_copies == 1 || r.bell_copies == 8) && (r.bell_copies == 1 || r.forward == 0), "resident: %d doorbell copies, forward %d", r.bell_copies, r.forward);
    REQUIRE(r.host_bell && r.host_lines && r.host_state && r.dev_quit && r.dev_bell && r.idle_ticks > 0 && r.life_ticks > 0 && r.max_calls > 0, "resident: arguments");
    REQUIRE(s != nullptr, "resident: launched on the default stream");
    hostsim::attach_worker(s, std::thread(resident_device, a, cfg, r));
    return hipSuccess;
}

} // namespace gat
