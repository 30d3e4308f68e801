// gat_acq_plan.h -- the pure part of gat_acquire (include/gat.h), the direct search: the call check it shares with gat_acquire_fft,
// its own refusals, the grid's tiles, the (antenna, block) unit groups and the scratch carve-up, as a function of the descriptor, the
// configuration and the device's compute-unit count alone.  No HIP call and no HIP header: the device entry point
// (gat_acq_api.cpp), the kernels (gat_acq.hip, through gat_acq_kernels.h) and a stand-alone test program (tests/acqplan) compile the
// same text.
//
// One edge is not the plan's: a grid of more than 65535 * kAcqDopTile Doppler bins passes every check here and is refused by the
// launch itself (grid.y beyond the device's limit), with the HIP error's code.
#pragma once

#include <algorithm>
#include <cmath>

#include "gat_acq_check.h"

namespace gat {

// the grid kernel's geometry
constexpr int kAcqThreads = 256;    // four wave64
constexpr int kAcqDopPerWave = 8;   // Doppler bins of one wave's register tile
constexpr int kAcqCodePerLane = 4;  // code bins of one lane's register tile (lane + 64 r)
constexpr int kAcqDopTile = kAcqDopPerWave * (kAcqThreads / 64); // 32 Doppler bins per workgroup
constexpr int kAcqCodeTile = kAcqCodePerLane * 64;               // 256 code bins per workgroup
constexpr int kAcqChunk = 128;      // samples staged per step (a power of two dividing kAcqThreads)

constexpr size_t kAcqMaxGroupScratch = (size_t)1 << 30; // bytes of the groups' slices
constexpr int kAcqMaxGridZ = 65535;                      // workgroups along the grid's (PRN, group) axis

// The call check both searches make before planning, after what needs the context: the configuration's refusals, code_length
// filled in from the bound table (0) and held to it, the block count, every PRN a row of the table (table_prns rows of
// table_length chips).  *cfg, the normalised configuration, is written only with GAT_OK.
inline Refusal acq_check_call(const gat_acq_config *cfg_in, int32_t B, const int32_t *prns, int32_t P, double fs, int32_t table_length,
                              int32_t table_prns, gat_acq_config *cfg)
{
    if (!cfg_in) return {GAT_ERR_ARG, "null config"};
    const Refusal r = acq_check_config(cfg_in, P, cfg_in->num_doppler_bins, cfg_in->num_code_bins, fs);
    if (r.code != GAT_OK) return r;
    gat_acq_config k = *cfg_in;
    k.struct_size = sizeof(gat_acq_config);
    if (k.code_length == 0) k.code_length = table_length;
    if (k.code_length != table_length) return {GAT_ERR_ARG, "config.code_length differs from the bound code table"};
    if (B < 1) return {GAT_ERR_ARG, "num_blocks must be positive"};
    for (int p = 0; p < P; ++p)
        if (prns[p] < 0 || prns[p] >= table_prns) return {GAT_ERR_RANGE, "prn outside the code table"};
    *cfg = k;
    return {GAT_OK, nullptr};
}

// What the tail of both searches reads in the context's scratch: the result records, the power grid (no caller's buffer), the
// unit groups' slices (several groups) and the PRN list, as byte offsets, and the whole call's bytes.
struct AcqScratch {
    size_t off_res, off_pow, off_part, off_prn, bytes;
};

// Units u = b M + m are dealt to G groups, u to group u mod G; a group's workgroups, one per (PRN, Doppler tile, code tile), sum its
// units in order into a slice of their own (G > 1), and the slices are added in group order.
struct AcqPlan : AcqScratch {
    int jtiles, dtiles; // the grid's tiles of kAcqCodeTile code bins and kAcqDopTile Doppler bins: the launcher's grid.x, grid.y
    int G;
    long long cells;    // P D J
    double reach;       // bound on every replica sample index the tiles' windows touch, unused code bins included
};

// The direct search's plan for a call that acq_check_call has passed (cfg: its normalised configuration, whose code_length is the
// table's).  *plan is written only with GAT_OK.
inline Refusal acq_plan(const gat_signal_desc *sig, int32_t B, int32_t P, double fs, const gat_acq_config *cfg, int num_cus, bool own_power,
                        AcqPlan *plan)
{
    const Refusal r = check_desc(sig, B, 0, signal_refusals({GAT_ERR_ARG, "chan_stride must be 0 (one signal for every PRN)"}));
    if (r.code != GAT_OK) return r;
    const int D = cfg->num_doppler_bins, J = cfg->num_code_bins, s = cfg->code_step_samples;
    AcqPlan p{};
    p.jtiles = (J + kAcqCodeTile - 1) / kAcqCodeTile, p.dtiles = (D + kAcqDopTile - 1) / kAcqDopTile;
    p.reach = (double)sig->num_samples + kAcqChunk + std::fabs((double)cfg->first_shift) + (double)s * p.jtiles * kAcqCodeTile;
    if (!(p.reach < 1073741824.0)) return {GAT_ERR_RANGE, "N + |first_shift| + s * J must stay below 2^30 samples"};
    if (code_span_bad(cfg->code_freq_hz / fs, (double)cfg->code_length, p.reach, cfg->code_length)) return {GAT_ERR_RANGE, "code phase span too large"};

    // groups of (antenna, block) units: enough workgroups for two per compute unit, within the scratch bound and the grid's z axis
    p.cells = (long long)P * D * J;
    const long long units = (long long)sig->num_ants * B, wgs = (long long)P * p.jtiles * p.dtiles;
    long long G = std::min(units, std::max(1ll, (2ll * num_cus + wgs - 1) / wgs));
    G = std::min(G, std::max(1ll, (long long)(kAcqMaxGroupScratch / ((size_t)p.cells * sizeof(float)))));
    G = std::min<long long>(G, kAcqMaxGridZ / P);
    if (G < 1) return {GAT_ERR_RANGE, "too many PRNs for one call"};
    p.G = (int)G;

    // scratch: [256 bytes | results | power (no caller's buffer), from a multiple of 256 bytes on | slices (G > 1) | prns]
    p.off_res = 256;
    p.off_pow = (p.off_res + (size_t)P * sizeof(gat_acq_result) + 255) & ~(size_t)255;
    p.off_part = p.off_pow + (own_power ? ((size_t)p.cells * sizeof(float) + 255) & ~(size_t)255 : 0);
    p.off_prn = p.off_part + (G > 1 ? (size_t)G * (size_t)p.cells * sizeof(float) : 0);
    p.bytes = p.off_prn + (size_t)P * sizeof(int32_t);
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
