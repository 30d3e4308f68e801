// gat_cond_plan.h -- the pure part of gat_condition_samples (include/gat.h): its refusals, the choice between the streaming and
// the general kernel and the work split, as a function of the two descriptors alone.  No HIP call and no HIP header: the
// device entry point, the host twin and a stand-alone test program (tests/condplan) compile the same text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "gat.h"

namespace gat {

constexpr int kCondThreads = 256;
constexpr int kCondStreamMaxAnts = 8; // the streaming kernel holds every antenna's 16-byte loads of a step up to here

constexpr int cond_sample_bytes(int fmt) // of one complex sample; planar: of one plane's float
{
    return fmt == GAT_LAYOUT_PLANAR ? 4 : fmt == GAT_LAYOUT_INTERLEAVED ? 8 : fmt == GAT_LAYOUT_INTERLEAVED_I16 ? 4 : 2;
}
constexpr int cond_vec_samples(int fmt) { return 16 / cond_sample_bytes(fmt); } // samples of one 16-byte load or store
// samples a lane of the streaming kernel owns per step: whole 16-byte loads AND whole 16-byte stores -- 8 where either side is
// int8 pairs (a float input then takes two loads per antenna and plane, ComplexF32 four), else 4
constexpr int cond_group_samples(int fmt_in, int fmt_out)
{
    return fmt_in == GAT_LAYOUT_INTERLEAVED_I8 || fmt_out == GAT_LAYOUT_INTERLEAVED_I8 ? 8 : 4;
}

// Work units are (block, chunk of `chunk` samples), `chunks` to a block, unit u = block * chunks + chunk index; workgroup g of
// `grid` takes units g, g + grid, ...  stream: chunk is a multiple of group * kCondThreads, so only a block's end is ragged.
struct CondPlan {
    bool stream, in_place;
    int group; // samples per lane and step (1: the general kernel)
    long long chunk, chunks, units, grid;
};

struct CondRefusal {
    int32_t code;
    const char *msg;
};

// unit u of a plan over blocks of N samples: its block and its samples [n0, n1)
#if defined(__HIPCC__)
__host__ __device__
#endif
inline void cond_unit(long long u, long long chunks, long long chunk, long long N, long long *b, long long *n0, long long *n1)
{
    *b = u / chunks;
    *n0 = (u - *b * chunks) * chunk;
    *n1 = *n0 + chunk < N ? *n0 + chunk : N;
}

namespace cond_detail {

inline double extent_samples(const gat_signal_desc *d, int B)
{
    return (double)(B - 1) * (double)d->block_stride + (double)(d->num_ants - 1) * (double)d->ant_stride + (double)d->num_samples;
}
struct ByteRange {
    uintptr_t lo, hi; // [lo, hi)
};
inline bool overlap(const ByteRange &a, const ByteRange &b) { return a.lo < b.hi && b.lo < a.hi; }
inline int plane_ranges(const gat_signal_desc *d, int B, ByteRange (&r)[2])
{
    const bool planar = d->layout == GAT_LAYOUT_PLANAR;
    const uintptr_t bytes = (uintptr_t)extent_samples(d, B) * (uintptr_t)cond_sample_bytes(d->layout);
    r[0] = {reinterpret_cast<uintptr_t>(d->re), reinterpret_cast<uintptr_t>(d->re) + bytes};
    r[1] = r[0];
    if (planar) r[1] = {reinterpret_cast<uintptr_t>(d->im), reinterpret_cast<uintptr_t>(d->im) + bytes};
    return planar ? 2 : 1;
}
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// every block of every antenna starts on a 16-byte boundary (the fast-path rule of gat.h)
inline bool blocks_aligned(const gat_signal_desc *d, int B)
{
    const long long vs = cond_vec_samples(d->layout);
    return aligned16(d->re) && (d->layout != GAT_LAYOUT_PLANAR || aligned16(d->im)) && (d->num_ants == 1 || d->ant_stride % vs == 0) &&
           (B == 1 || d->block_stride % vs == 0);
}
inline CondRefusal check_side(const gat_signal_desc *d, int B, const char *planes, const char *sizes, const char *ants, const char *blocks)
{
    if (d->layout < GAT_LAYOUT_PLANAR || d->layout > GAT_LAYOUT_INTERLEAVED_I8) return {GAT_ERR_ARG, "bad layout"};
    if (!d->re || (d->layout == GAT_LAYOUT_PLANAR) != (d->im != nullptr)) return {GAT_ERR_ARG, planes};
    if (d->num_ants < 1 || d->num_samples < 1 || d->ant_stride < 0 || d->block_stride < 0) return {GAT_ERR_ARG, sizes};
    if (d->num_ants > 1 && d->ant_stride < 1) return {GAT_ERR_ARG, ants};
    if (B > 1 && d->block_stride < 1) return {GAT_ERR_ARG, blocks};
    return {GAT_OK, nullptr};
}

} // namespace cond_detail

// The signal side alone (what gat_sample_stats shares): GAT_OK or the refusal
inline CondRefusal cond_check_signal(const gat_signal_desc *sig, int32_t B)
{
    using namespace cond_detail;
    if (!sig) return {GAT_ERR_ARG, "null argument"};
    if (B < 1) return {GAT_ERR_ARG, "num_blocks must be positive"};
    const CondRefusal r = check_side(sig, B, "bad signal planes", "bad signal sizes", "ant_stride must be positive", "block_stride must be positive");
    if (r.code != GAT_OK) return r;
    if (sig->num_ants > GAT_MAX_ARRAY_ANTS) return {GAT_ERR_RANGE, "more than 64 antennas"};
    if (sig->chan_stride != 0) return {GAT_ERR_UNSUPPORTED, "chan_stride must be 0"};
    if (extent_samples(sig, B) > 9.0e15) return {GAT_ERR_RANGE, "signal extent too large"};
    return {GAT_OK, nullptr};
}

// The whole call.  workgroups_wanted: about eight a compute unit on the device.  *plan is written only with GAT_OK.
inline CondRefusal cond_plan(const gat_signal_desc *sig, int32_t B, const void *params, uint32_t flags, const gat_signal_desc *out,
                             long long workgroups_wanted, CondPlan *plan)
{
    using namespace cond_detail;
    if (!sig || !out || !params || !plan) return {GAT_ERR_ARG, "null argument"};
    if (flags & ~(uint32_t)GAT_COND_BLANK_ALL_ANTS) return {GAT_ERR_ARG, "unknown flags"};
    CondRefusal r = cond_check_signal(sig, B);
    if (r.code != GAT_OK) return r;
    r = check_side(out, B, "bad output planes", "bad output sizes", "the output's ant_stride must be positive",
                   "the output's block_stride must be positive");
    if (r.code != GAT_OK) return r;
    if (out->num_ants != sig->num_ants) return {GAT_ERR_ARG, "the output's num_ants must be the signal's"};
    if (out->num_samples != sig->num_samples) return {GAT_ERR_ARG, "the output's num_samples must be the signal's"};
    if (out->chan_stride != 0) return {GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides"};
    if (extent_samples(out, B) > 9.0e15) return {GAT_ERR_RANGE, "signal extent too large"};
    const int M = sig->num_ants;
    // in place: the same elements at the same addresses, so that every lane reads what it is about to overwrite and nothing else
    const bool same = out->layout == sig->layout && out->re == sig->re && out->im == sig->im && (M == 1 || out->ant_stride == sig->ant_stride) &&
                      (B == 1 || out->block_stride == sig->block_stride);
    if (!same) {
        ByteRange in_r[2], out_r[2];
        const int in_n = plane_ranges(sig, B, in_r), out_n = plane_ranges(out, B, out_r);
        for (int i = 0; i < in_n; ++i)
            for (int o = 0; o < out_n; ++o)
                if (overlap(in_r[i], out_r[o])) return {GAT_ERR_ARG, "the output overlaps the signal without being identical to it"};
    }

    CondPlan p{};
    p.in_place = same;
    p.stream = M <= kCondStreamMaxAnts && blocks_aligned(sig, B) && blocks_aligned(out, B);
    p.group = p.stream ? cond_group_samples(sig->layout, out->layout) : 1;
    // about workgroups_wanted work units, a chunk no shorter than four steps of a workgroup
    const long long N = sig->num_samples, round_to = (long long)kCondThreads * p.group;
    const long long want = workgroups_wanted < 1 ? 1 : workgroups_wanted;
    long long chunks = 1;
    if (B < want) {
        const long long by_want = (want + B - 1) / B, by_len = N / (4 * round_to) < 1 ? 1 : N / (4 * round_to);
        chunks = by_want < by_len ? by_want : by_len;
    }
    p.chunk = ((N + chunks - 1) / chunks + round_to - 1) / round_to * round_to;
    p.chunks = (N + p.chunk - 1) / p.chunk;
    p.units = (long long)B * p.chunks; // chunks > 1 only where B < want: below 2^31 either way
    p.grid = p.units < want ? p.units : want;
    *plan = p;
    return {GAT_OK, nullptr};
}

} // namespace gat
