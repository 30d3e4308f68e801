// gat_sig_plan.h -- the host-side rules that the operators over a gat_signal_desc of raw samples share (gat_spatial_covariance,
// gat_beamform_samples, gat_sample_stats, gat_condition_samples, gat_acquire, the correlator's planner), each stated once, as pure
// functions of descriptors and sizes, and with them the host's read of one sample and the launchers' layout dispatch.  No HIP call
// and no HIP header: the device entry points, the operators' pure plans (gat_cond_plan.h, gat_beam_plan.h) and the stand-alone
// test programs (tests/condplan and its kin) compile the same text.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "gat.h"

namespace gat {

// Layout arithmetic.  Bytes of one sample in one plane: planar f32 4, interleaved ComplexF32 8, interleaved int16 4,
// interleaved int8 2 -- and the samples one 16-byte load or store holds: 4, 2, 4, 8.
constexpr int layout_sample_bytes(int fmt)
{
    return fmt == GAT_LAYOUT_PLANAR ? 4 : fmt == GAT_LAYOUT_INTERLEAVED ? 8 : fmt == GAT_LAYOUT_INTERLEAVED_I16 ? 4 : 2;
}
constexpr int layout_vec_samples(int fmt) { return 16 / layout_sample_bytes(fmt); }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Host access to sample e of a descriptor's memory (the host twins; the kernels' reads are gat_sample_load.h).
inline void host_load_sample(const gat_signal_desc *d, size_t e, float *xr, float *xi)
{
    switch (d->layout) {
    case GAT_LAYOUT_PLANAR: *xr = static_cast<const float *>(d->re)[e], *xi = static_cast<const float *>(d->im)[e]; break;
    case GAT_LAYOUT_INTERLEAVED: *xr = static_cast<const float *>(d->re)[2 * e], *xi = static_cast<const float *>(d->re)[2 * e + 1]; break;
    case GAT_LAYOUT_INTERLEAVED_I16: *xr = (float)static_cast<const int16_t *>(d->re)[2 * e], *xi = (float)static_cast<const int16_t *>(d->re)[2 * e + 1]; break;
    default: *xr = (float)static_cast<const int8_t *>(d->re)[2 * e], *xi = (float)static_cast<const int8_t *>(d->re)[2 * e + 1]; break;
    }
}

// A runtime layout as a compile-time one: calls f(std::integral_constant<int, GAT_LAYOUT_*>), which a launcher hands on as a
// template argument.  A value outside the four goes the int8 way; the plans have refused it before any launcher is reached.
template <class F>
decltype(auto) dispatch_layout(int fmt, F &&f)
{
    switch (fmt) {
    case GAT_LAYOUT_PLANAR: return f(std::integral_constant<int, GAT_LAYOUT_PLANAR>{});
    case GAT_LAYOUT_INTERLEAVED: return f(std::integral_constant<int, GAT_LAYOUT_INTERLEAVED>{});
    case GAT_LAYOUT_INTERLEAVED_I16: return f(std::integral_constant<int, GAT_LAYOUT_INTERLEAVED_I16>{});
    default: return f(std::integral_constant<int, GAT_LAYOUT_INTERLEAVED_I8>{});
    }
}

// What planning returns: GAT_OK, or a refusal's code and message (the caller reports it with fail()).
struct Refusal {
    int32_t code;
    const char *msg;
};

// samples from the first to one past the last element a descriptor covers over B blocks, and every operator's bound on it
constexpr double kMaxExtentSamples = 9.0e15;
inline double extent_samples(const gat_signal_desc *d, int B)
{
    return (double)(B - 1) * (double)d->block_stride + (double)(d->num_ants - 1) * (double)d->ant_stride + (double)d->num_samples;
}

// The fast-path rule of gat.h: every block of every antenna starts on a 16-byte boundary (a stride never applied does not matter)
inline bool blocks_aligned(const gat_signal_desc *d, int B)
{
    const long long vs = layout_vec_samples(d->layout);
    return aligned16(d->re) && (d->layout != GAT_LAYOUT_PLANAR || aligned16(d->im)) && (d->num_ants == 1 || d->ant_stride % vs == 0) &&
           (B == 1 || d->block_stride % vs == 0);
}

// the byte ranges of a checked descriptor's planes (the interleaved layouts: the one plane twice), and whether a's meet b's
struct ByteRange {
    uintptr_t lo, hi; // [lo, hi)
};
inline void plane_ranges(const gat_signal_desc *d, int B, ByteRange (&r)[2])
{
    const uintptr_t bytes = (uintptr_t)extent_samples(d, B) * (uintptr_t)layout_sample_bytes(d->layout);
    const uintptr_t re = reinterpret_cast<uintptr_t>(d->re), im = d->layout == GAT_LAYOUT_PLANAR ? reinterpret_cast<uintptr_t>(d->im) : re;
    r[0] = {re, re + bytes}, r[1] = {im, im + bytes};
}
inline bool descs_overlap(const gat_signal_desc *a, const gat_signal_desc *b, int B)
{
    ByteRange ra[2], rb[2];
    plane_ranges(a, B, ra), plane_ranges(b, B, rb);
    for (const ByteRange &x : ra)
        for (const ByteRange &y : rb)
            if (x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}

// The descriptor check: a caller's answers to its findings, in the order check_desc looks for them (max_ants 0: no limit)
struct DescRefusals {
    Refusal layout, planes, sizes, ant_stride, block_stride, ants, chan_stride, extent;
};
// the signal side's answers: the operators differ in what they say about chan_stride alone
constexpr DescRefusals signal_refusals(Refusal chan_stride)
{
    return {{GAT_ERR_ARG, "bad layout"}, {GAT_ERR_ARG, "bad signal planes"}, {GAT_ERR_ARG, "bad signal sizes"},
            {GAT_ERR_ARG, "ant_stride must be positive"}, {GAT_ERR_ARG, "block_stride must be positive"},
            {GAT_ERR_RANGE, "more than 64 antennas"}, chan_stride, {GAT_ERR_RANGE, "signal extent too large"}};
}
inline Refusal check_desc(const gat_signal_desc *d, int B, int max_ants, const DescRefusals &t)
{
    if (d->layout < GAT_LAYOUT_PLANAR || d->layout > GAT_LAYOUT_INTERLEAVED_I8) return t.layout;
    if (!d->re || (d->layout == GAT_LAYOUT_PLANAR) != (d->im != nullptr)) return t.planes;
    if (d->num_ants < 1 || d->num_samples < 1 || d->ant_stride < 0 || d->block_stride < 0) return t.sizes;
    if (d->num_ants > 1 && d->ant_stride < 1) return t.ant_stride;
    if (B > 1 && d->block_stride < 1) return t.block_stride;
    if (max_ants > 0 && d->num_ants > max_ants) return t.ants;
    if (d->chan_stride != 0) return t.chan_stride; // these operators read one signal
    if (extent_samples(d, B) > kMaxExtentSamples) return t.extent;
    return {GAT_OK, nullptr};
}

// The (estimate, block, segment) work split.  An estimate of `blocks` blocks gets G <= per_est workgroups; its work units are (block,
// segment of seg_len samples: a multiple of round_to, min_seg or more where a block is cut), `splits` to a block; workgroup g takes g, g + G, ...
struct EstimateSplit {
    long long splits, seg_len, G;
};
inline EstimateSplit split_estimate(long long blocks, long long N, long long round_to, long long min_seg, long long per_est)
{
    long long splits = 1;
    if (blocks < per_est) {
        const long long by_want = (per_est + blocks - 1) / blocks, by_len = N / min_seg < 1 ? 1 : N / min_seg;
        splits = by_want < by_len ? by_want : by_len;
    }
    const long long seg_len = ((N + splits - 1) / splits + round_to - 1) / round_to * round_to;
    splits = (N + seg_len - 1) / seg_len;
    return {splits, seg_len, blocks * splits < per_est ? blocks * splits : per_est};
}

// The (block, chunk) work split: the same with the whole call as its one estimate and four steps of a workgroup (round_to) as the
// shortest chunk.  Unit u = block * chunks + chunk index, `chunk` samples each; workgroup g of `grid` (about `want`) takes g, g + grid, ...
struct ChunkSplit {
    long long chunk, chunks, units, grid;
};
inline ChunkSplit split_chunks(long long B, long long N, long long round_to, long long want)
{
    const EstimateSplit s = split_estimate(B, N, round_to, 4 * round_to, want < 1 ? 1 : want);
    return {s.seg_len, s.splits, B * s.splits, s.G}; // chunks > 1 only where B < want: units below 2^31 either way
}

// bytes from a plane's start to block b0 of a descriptor (a batch of an estimating call's launches: gat_est_plan.h)
inline size_t block_offset_bytes(const gat_signal_desc *d, int b0)
{
    return (size_t)b0 * (size_t)d->block_stride * (size_t)layout_sample_bytes(d->layout);
}

} // namespace gat
