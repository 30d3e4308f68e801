// gat_beam_api.cpp -- host side of gat_beamform_samples (include/gat.h): validation, the choice between the streaming and the
// general kernel, the work split, the launches.  The kernels are gat_beam.hip.
#include <algorithm>

#include "gat_beam_kernels.h"
#include "gat_ctx.h"

using namespace gat;

namespace {

// samples from the first to one past the last element a descriptor covers
double extent_samples(const gat_signal_desc *d, int B)
{
    return (double)(B - 1) * (double)d->block_stride + (double)(d->num_ants - 1) * (double)d->ant_stride + (double)d->num_samples;
}

struct ByteRange {
    uintptr_t lo, hi; // [lo, hi)
};
inline bool overlap(const ByteRange &a, const ByteRange &b) { return a.lo < b.hi && b.lo < a.hi; }

// the byte ranges of a descriptor's planes (one for the interleaved layouts)
int plane_ranges(const gat_signal_desc *d, int B, ByteRange (&r)[2])
{
    const bool planar = d->layout == GAT_LAYOUT_PLANAR;
    const uintptr_t bytes = (uintptr_t)extent_samples(d, B) * (uintptr_t)(planar ? 4 : layout_sample_bytes(d->layout));
    r[0] = {reinterpret_cast<uintptr_t>(d->re), reinterpret_cast<uintptr_t>(d->re) + bytes};
    if (planar) r[1] = {reinterpret_cast<uintptr_t>(d->im), reinterpret_cast<uintptr_t>(d->im) + bytes};
    return planar ? 2 : 1;
}

} // namespace

GAT_API int32_t gat_beamform_samples(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const double *w_re, const double *w_im, int32_t J,
                                     const gat_signal_desc *out)
{
    if (!c) return GAT_ERR_ARG;
    if (!sig || !out || !w_re || !w_im) return fail(c, GAT_ERR_ARG, "null argument");
    if (B < 1 || J < 1) return fail(c, GAT_ERR_ARG, "num_blocks and num_beams must be positive");
    const int layout = sig->layout;
    if (layout < GAT_LAYOUT_PLANAR || layout > GAT_LAYOUT_INTERLEAVED_I8) return fail(c, GAT_ERR_ARG, "bad layout");
    if (!sig->re || (layout == GAT_LAYOUT_PLANAR) != (sig->im != nullptr)) return fail(c, GAT_ERR_ARG, "bad signal planes");
    if (sig->num_ants < 1 || sig->num_samples < 1 || sig->ant_stride < 0 || sig->block_stride < 0) return fail(c, GAT_ERR_ARG, "bad signal sizes");
    if (out->ant_stride < 0 || out->block_stride < 0) return fail(c, GAT_ERR_ARG, "negative output stride");
    if (sig->num_ants > GAT_MAX_ARRAY_ANTS) return fail(c, GAT_ERR_RANGE, "more than 64 antennas");
    if (J > GAT_MAX_ARRAY_ANTS) return fail(c, GAT_ERR_RANGE, "more than 64 beams");
    if (out->num_ants != J) return fail(c, GAT_ERR_ARG, "the output's num_ants must be num_beams");
    if (out->num_samples != sig->num_samples) return fail(c, GAT_ERR_ARG, "the output's num_samples must be the signal's");
    if (out->layout == GAT_LAYOUT_INTERLEAVED_I16 || out->layout == GAT_LAYOUT_INTERLEAVED_I8)
        return fail(c, GAT_ERR_UNSUPPORTED, "the output is float32: planar or interleaved");
    if (out->layout != GAT_LAYOUT_PLANAR && out->layout != GAT_LAYOUT_INTERLEAVED) return fail(c, GAT_ERR_ARG, "bad output layout");
    if (sig->chan_stride != 0 || out->chan_stride != 0) return fail(c, GAT_ERR_UNSUPPORTED, "chan_stride must be 0 on both sides");
    const bool out_planar = out->layout == GAT_LAYOUT_PLANAR;
    if (!out->re || out_planar != (out->im != nullptr)) return fail(c, GAT_ERR_ARG, "bad output planes");
    const int M = sig->num_ants;
    if (M > 1 && sig->ant_stride < 1) return fail(c, GAT_ERR_ARG, "ant_stride must be positive");
    if (B > 1 && (sig->block_stride < 1 || out->block_stride < 1)) return fail(c, GAT_ERR_ARG, "block_stride must be positive");
    if (J > 1 && out->ant_stride < 1) return fail(c, GAT_ERR_ARG, "the output's ant_stride must be positive");
    if (extent_samples(sig, B) > 9.0e15 || extent_samples(out, B) > 9.0e15) return fail(c, GAT_ERR_RANGE, "signal extent too large");
    ByteRange in_r[2], out_r[2];
    const int in_n = plane_ranges(sig, B, in_r), out_n = plane_ranges(out, B, out_r);
    for (int i = 0; i < in_n; ++i)
        for (int o = 0; o < out_n; ++o)
            if (overlap(in_r[i], out_r[o])) return fail(c, GAT_ERR_ARG, "the output overlaps the signal");

    // the streaming kernel's rule: every block of every antenna (the correlator's fast-path rule) and of every beam starts
    // on a 16-byte boundary
    const long long vs = layout_vec_samples(layout), ovs = out_planar ? 4 : 2;
    const bool stream = M <= kBeamStreamMaxAnts && aligned16(sig->re) && (layout != GAT_LAYOUT_PLANAR || aligned16(sig->im)) &&
                        (M == 1 || sig->ant_stride % vs == 0) && (B == 1 || sig->block_stride % vs == 0) && aligned16(out->re) &&
                        (!out_planar || aligned16(out->im)) && (J == 1 || out->ant_stride % ovs == 0) && (B == 1 || out->block_stride % ovs == 0);

    // work units (block, chunk): about eight workgroups a CU, a chunk no shorter than four steps of a workgroup
    const long long N = sig->num_samples;
    const long long round_to = (long long)kBeamThreads * (stream ? beam_group_samples(layout) : 1);
    const long long want = (long long)c->num_cus * 8;
    long long chunks = 1;
    if (B < want) chunks = std::min<long long>((want + B - 1) / B, std::max<long long>(1, N / (4 * round_to)));
    const long long chunk = ((N + chunks - 1) / chunks + round_to - 1) / round_to * round_to;
    chunks = (N + chunk - 1) / chunk;
    const long long grid = std::min<long long>((long long)B * chunks, want); // chunks > 1 only where B < want: B * chunks < 2^31

    GAT_ENTER(c, "gat_beamform_samples");
    const int T = beam_tile(stream, J);
    const int32_t rc = ensure_partial(c, beam_weight_count(J, M, T) * sizeof(float2));
    if (rc != GAT_OK) return rc;
    float2 *w32 = reinterpret_cast<float2 *>(c->d_partial);
    BeamArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.out_re = static_cast<float *>(const_cast<void *>(out->re));
    a.out_im = static_cast<float *>(const_cast<void *>(out->im));
    a.M = M;
    a.B = B;
    a.J = J;
    a.chunks = (int)chunks;
    a.N = N;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.out_ant_stride = out->ant_stride;
    a.out_block_stride = out->block_stride;
    a.chunk = chunk;
    GAT_HIP(c, launch_beam_weights(w_re, w_im, J, M, T, w32, c->stream));
    GAT_HIP(c, stream ? launch_beam_stream(a, layout, w32, (int)grid, c->stream) : launch_beam_general(a, layout, w32, (int)grid, c->stream));
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)grid;
    c->last.threads = kBeamThreads;
    c->last.splits = (int32_t)chunks;
    c->last.ant_tile = M;
    c->last.vec = stream ? 4 : 1;
    // the weights in LDS: the general kernel's [64][T] float2; the streaming kernel's [M][T] when T > 1 (one beam: scalar loads, no LDS)
    c->last.lds_bytes = (int32_t)sizeof(float2) * (stream ? (T > 1 ? M * T : 0) : GAT_MAX_ARRAY_ANTS * T);
    return GAT_OK;
}
