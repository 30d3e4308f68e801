// gat_spec_plan.h -- the pure part of gat_sample_spectrum (include/gat.h): its refusals, the choice between the aligned and the
// general load path, the kernel's geometry and the work split, as a function of the descriptor and the configuration alone.  No
// HIP call and no HIP header: the device entry point, the host twin and a stand-alone test program (tests/specplan) compile the
// same text.
#pragma once

#include "gat_sig_plan.h"
#include "gat_hd.h"

namespace gat {

constexpr int kSpecThreads = 256;
constexpr int kSpecMinLanePoints = 4; // points a lane keeps in registers at least: two stages between trips through LDS

// The kernel's geometry.  A lane keeps R = max(4, F / 256) points, so a transform takes a TEAM of F / R lanes (16 .. 256) and a
// workgroup holds 256 / team teams, each with a work unit of its own: no lane idles at a small F.  The stages run in passes of
// log2 R stages between trips through LDS (the first pass takes what log2 F leaves over: 1 .. log2 R stages).
constexpr int spec_lane_points(int F) { return F / kSpecThreads > kSpecMinLanePoints ? F / kSpecThreads : kSpecMinLanePoints; }
constexpr int spec_ilog2(int v) { return v <= 1 ? 0 : 1 + spec_ilog2(v / 2); }

// Where register i (< R) of lane t (< team) lies in the transform's array during a pass of rs stages from stage j on: the rs
// low bits of i are the pass's butterfly bits, at bit j of the index; the other bits of i extend the lane's number.  *v, *ii:
// the extended lane number and the butterfly bits (the twiddle of stage j + q is number ((ii mod 2^q) << j | v mod 2^j) << (L - 1 - j - q)).
GAT_HD inline unsigned spec_point_index(unsigned t, unsigned i, int R, int j, int rs, unsigned *v, unsigned *ii)
{
    *v = t * (unsigned)(R >> rs) + (i >> rs);
    *ii = i & ((1u << rs) - 1u);
    return ((*v >> j) << (j + rs)) | (*ii << j) | (*v & ((1u << j) - 1u));
}

// The skew of the point and the twiddle arrays in LDS: the low five bits (the bank of an 8-byte element, 32 to a bank row) XORed
// with the next two five-bit digits.  A bijection of [0, F) for F >= 32; lanes whose indices differ in five neighbouring bits, as
// power-of-two strides make them, fall on 32 different banks (scripts/spectrum_lds_model.py counts every access).
GAT_HD inline unsigned spec_skew(unsigned p) { return p ^ ((p >> 5) & 31u) ^ ((p >> 10) & 31u); }

// Work units are (block, antenna) pairs: unit u = block * M + antenna.  A workgroup takes `teams` consecutive units at a time (a
// round): round r = units [r * teams, (r + 1) * teams); workgroup g of `grid` takes rounds g, g + grid, ...
struct SpecPlan {
    bool aligned;     // 16-byte loads
    int log2F, R, team, teams;
    long long S, units, rounds, grid;
};

GAT_HD inline void spec_unit(long long u, int M, long long *b, int *m)
{
    *b = u / M;
    *m = (int)(u - *b * M);
}

// The whole call.  workgroups_wanted: what fills the device.  *plan is written only with GAT_OK.
inline Refusal spec_plan(const gat_signal_desc *sig, int32_t B, const float *window, const gat_spectrum_config *cfg, const float *power,
                         long long workgroups_wanted, SpecPlan *plan)
{
    if (!sig || !window || !cfg || !power || !plan) return {GAT_ERR_ARG, "null argument"};
    if (cfg->struct_size != sizeof(gat_spectrum_config)) return {GAT_ERR_ARG, "struct_size is not sizeof(gat_spectrum_config)"};
    if (B < 1) return {GAT_ERR_ARG, "num_blocks must be positive"};
    if (cfg->flags != 0) return {GAT_ERR_ARG, "flags must be 0"};
    const int F = cfg->num_bins, H = cfg->hop;
    if (F < GAT_MIN_SPECTRUM_BINS || F > GAT_MAX_SPECTRUM_BINS || (F & (F - 1)) != 0) return {GAT_ERR_RANGE, "num_bins must be a power of two in 64 .. 4096"};
    if (H < 1 || H > F) return {GAT_ERR_RANGE, "hop outside 1 .. num_bins"};
    const Refusal r = check_desc(sig, B, GAT_MAX_ARRAY_ANTS, signal_refusals({GAT_ERR_UNSUPPORTED, "chan_stride must be 0"}));
    if (r.code != GAT_OK) return r;
    const long long N = sig->num_samples;
    if (N < F) return {GAT_ERR_ARG, "a block is shorter than one segment"};
    const long long S = (N - F) / H + 1;
    if (S > GAT_MAX_SPECTRUM_SEGMENTS) return {GAT_ERR_RANGE, "more than 4096 segments a block"};
    const int M = sig->num_ants;
    ByteRange in[2];
    plane_ranges(sig, B, in);
    const uintptr_t lo = reinterpret_cast<uintptr_t>(power), hi = lo + (uintptr_t)B * (uintptr_t)M * (uintptr_t)F * sizeof(float);
    for (const ByteRange &x : in)
        if (x.lo < hi && lo < x.hi) return {GAT_ERR_ARG, "the output overlaps the signal"};

    SpecPlan p{};
    p.aligned = blocks_aligned(sig, B) && H % layout_vec_samples(sig->layout) == 0;
    p.log2F = spec_ilog2(F);
    p.R = spec_lane_points(F);
    p.team = F / p.R;
    p.teams = kSpecThreads / p.team;
    p.S = S;
    p.units = (long long)B * M;
    p.rounds = (p.units + p.teams - 1) / p.teams;
    const long long want = workgroups_wanted < 1 ? 1 : workgroups_wanted;
    p.grid = p.rounds < want ? p.rounds : want;
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
