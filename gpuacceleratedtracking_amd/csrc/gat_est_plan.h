// gat_est_plan.h -- the work split of the operators that reduce blocks of raw samples to estimates (gat_spatial_covariance,
// gat_sample_stats, gat_spacetime_covariance): the rule of one call as data, and the one walk over the call's launches.  The
// operators' pure plans (gat_array_plan.h, gat_cond_plan.h, gat_st_plan.h) fill the rule in; the C ABI layer's enqueue loop
// (gat_ctx.h, enqueue_estimates) and a stand-alone test program (tests/estplan) walk it.  No HIP call, no HIP header and no heap:
// these calls run once per block batch in the closed loop and inside captured graphs.
#pragma once

#include <algorithm>

#include "gat_sig_plan.h"

namespace gat {

// The estimates of a call -- ceil(B / bpe), of bpe blocks each, the last one shorter -- in batches whose slices (slice_bytes an estimate
// and workgroup) fit cap_bytes of scratch with one workgroup an estimate at least: after next(), estimates [e0, e0 + en) own blocks [b0, b0 + bn).
struct EstimateBatches {
    const int B, bpe, E, e_max;
    int e0 = 0, en = 0, b0 = 0, bn = 0;
    EstimateBatches(int B_, int bpe_, size_t slice_bytes, size_t cap_bytes)
        : B(B_), bpe(bpe_), E((int)(((long long)B_ + bpe_ - 1) / bpe_)),
          e_max(cap_bytes / slice_bytes < 1 ? 1 : cap_bytes / slice_bytes > ((size_t)1 << 20) ? 1 << 20 : (int)(cap_bytes / slice_bytes)) {}
    bool next()
    {
        if ((e0 += en) >= E) return false;
        en = e_max < E - e0 ? e_max : E - e0;
        const long long first = (long long)e0 * bpe, most = (long long)en * bpe;
        b0 = (int)first;
        bn = (int)(B - first < most ? B - first : most);
        return true;
    }
};

// The rule of one estimating call: B blocks in estimates of bpe; N samples (or snapshots) of a block are what a split cuts, into
// segments that are multiples of round_to and min_seg or longer; a launch wants workgroups_wanted workgroups over its estimates;
// a workgroup's sums are a slice of slice_bytes, and a launch's slices stay within cap_bytes where one workgroup an estimate can.
struct EstimatePlan {
    int B, bpe;
    long long N, round_to, min_seg, workgroups_wanted;
    size_t slice_bytes, cap_bytes;
};

// The launches of a call, in order.  After next(): estimates [e0, e0 + en) own blocks [b0, b0 + bn) of the call, and the launch sees
// them as its blocks [0, bn): estimate e of it owns blocks [e * bpe, min(bn, (e + 1) * bpe)) and G workgroups, its units are (block
// u / splits, segment u % splits of seg_len), workgroup g takes units g, g + G, ...; scratch_bytes hold the launch's en * G slices.
struct EstimateLaunches : EstimateBatches {
    const EstimatePlan plan;
    long long G = 0, splits = 0, seg_len = 0;
    size_t scratch_bytes = 0;
    explicit EstimateLaunches(const EstimatePlan &p) : EstimateBatches(p.B, p.bpe, p.slice_bytes, p.cap_bytes), plan(p) {}
    bool next()
    {
        if (!EstimateBatches::next()) return false;
        const EstimateSplit sp =
            split_estimate(std::min(bpe, bn), plan.N, plan.round_to, plan.min_seg, std::max<long long>(1, plan.workgroups_wanted / en));
        G = sp.G, splits = sp.splits, seg_len = sp.seg_len;
        scratch_bytes = (size_t)en * (size_t)G * plan.slice_bytes;
        return true;
    }
};

} // namespace gat
