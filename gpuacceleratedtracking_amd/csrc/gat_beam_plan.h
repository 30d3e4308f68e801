// gat_beam_plan.h -- the pure part of gat_beamform_samples (include/gat.h): its refusals, the choice between the streaming and
// the general kernel and the work split, as a function of the call's arguments alone.  No HIP call and no HIP header: the
// device entry point and a stand-alone test program (tests/condplan) compile the same text.
#pragma once

#include "gat_sig_plan.h"

namespace gat {

constexpr int kBeamThreads = 256;
constexpr int kBeamStreamMaxAnts = 8; // the streaming kernel holds one 16-byte load per antenna (and plane) up to here

// samples a lane of the streaming kernel takes per step: whole 16-byte loads (4 / 2 / 4 / 8 samples by layout) AND whole 16-byte
// stores of either output layout (4 samples a plane, 2 interleaved) -- two loads per antenna for ComplexF32 pairs
constexpr int beam_group_samples(int fmt) { return fmt == GAT_LAYOUT_INTERLEAVED_I8 ? 8 : 4; }

// The work split is split_chunks' (gat_sig_plan.h).  stream: chunk is a multiple of group * kBeamThreads.
struct BeamPlan {
    bool stream;
    int group; // samples per lane and step (1: the general kernel)
    long long chunk, chunks, units, grid;
};

// The whole call.  workgroups_wanted: about eight a compute unit on the device.  *plan is written only with GAT_OK.
inline Refusal beam_plan(const gat_signal_desc *sig, int32_t B, const double *w_re, const double *w_im, int32_t J, const gat_signal_desc *out,
                         long long workgroups_wanted, BeamPlan *plan)
{
    // (a bad size of the output is caught as a difference from num_beams or from the signal: `sizes` is left a negative stride)
    constexpr DescRefusals kOutput{{GAT_ERR_ARG, "bad output layout"}, {GAT_ERR_ARG, "bad output planes"}, {GAT_ERR_ARG, "negative output stride"},
                                   {GAT_ERR_ARG, "the output's ant_stride must be positive"}, {GAT_ERR_ARG, "block_stride must be positive"},
                                   {GAT_ERR_RANGE, "more than 64 beams"}, {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"},
                                   {GAT_ERR_RANGE, "signal extent too large"}};
    if (!sig || !out || !w_re || !w_im || !plan) return {GAT_ERR_ARG, "null argument"};
    if (B < 1 || J < 1) return {GAT_ERR_ARG, "num_blocks and num_beams must be positive"};
    Refusal r = check_desc(sig, B, GAT_MAX_ARRAY_ANTS, signal_refusals({GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"}));
    if (r.code != GAT_OK) return r;
    if (J > GAT_MAX_ARRAY_ANTS) return kOutput.ants;
    if (out->num_ants != J) return {GAT_ERR_ARG, "the output's num_ants must be num_beams"};
    if (out->num_samples != sig->num_samples) return {GAT_ERR_ARG, "the output's num_samples must be the signal's"};
    if (out->layout == GAT_LAYOUT_INTERLEAVED_I16 || out->layout == GAT_LAYOUT_INTERLEAVED_I8)
        return {GAT_ERR_UNSUPPORTED, "the output is float32: planar or interleaved"};
    r = check_desc(out, B, GAT_MAX_ARRAY_ANTS, kOutput);
    if (r.code != GAT_OK) return r;
    if (descs_overlap(sig, out, B)) return {GAT_ERR_ARG, "the output overlaps the signal"};

    // the streaming kernel's rule: every block of every antenna and of every beam starts on a 16-byte boundary
    BeamPlan p{};
    p.stream = sig->num_ants <= kBeamStreamMaxAnts && blocks_aligned(sig, B) && blocks_aligned(out, B);
    p.group = p.stream ? beam_group_samples(sig->layout) : 1;
    const ChunkSplit s = split_chunks(B, sig->num_samples, (long long)kBeamThreads * p.group, workgroups_wanted);
    p.chunk = s.chunk, p.chunks = s.chunks, p.units = s.units, p.grid = s.grid;
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
