// gat_cond_api.cpp -- host side of the sample conditioner (include/gat.h gat_condition_samples, gat_sample_stats,
// gat_agc_update): the launches behind the pure plans of gat_cond_plan.h, and the host twins
// (gat_condition_samples_host, gat_agc_update_host), which run the arithmetic of gat_cond.h in plain loops.
#include <algorithm>
#include <cmath>

#include "gat_cond.h"
#include "gat_cond_kernels.h"
#include "gat_ctx.h"

using namespace gat;

namespace {

bool agc_config_ok(const gat_agc_config *cfg)
{
    return cfg && cfg->struct_size == sizeof(gat_agc_config) && std::isfinite(cfg->target_rms) && cfg->target_rms >= 0.0 &&
           !std::isnan(cfg->blank_factor);
}

// one output sample by the rule; returns the clipped components
int host_store(const gat_signal_desc *d, size_t e, bool keep, float xr, float xi, const gat_cond_params &p)
{
    void *re = const_cast<void *>(d->re), *im = const_cast<void *>(d->im);
    const float yr = keep ? cond_value(xr, p.dc_re, p.scale) : 0.0f, yi = keep ? cond_value(xi, p.dc_im, p.scale) : 0.0f;
    if (d->layout == GAT_LAYOUT_PLANAR) {
        static_cast<float *>(re)[e] = yr, static_cast<float *>(im)[e] = yi;
        return 0;
    }
    if (d->layout == GAT_LAYOUT_INTERLEAVED) {
        static_cast<float *>(re)[2 * e] = yr, static_cast<float *>(re)[2 * e + 1] = yi;
        return 0;
    }
    const int lim = d->layout == GAT_LAYOUT_INTERLEAVED_I16 ? 32767 : 127;
    bool c_re = false, c_im = false;
    const int o_re = keep ? cond_code(yr, lim, &c_re) : 0, o_im = keep ? cond_code(yi, lim, &c_im) : 0;
    if (d->layout == GAT_LAYOUT_INTERLEAVED_I16)
        static_cast<int16_t *>(re)[2 * e] = (int16_t)o_re, static_cast<int16_t *>(re)[2 * e + 1] = (int16_t)o_im;
    else
        static_cast<int8_t *>(re)[2 * e] = (int8_t)o_re, static_cast<int8_t *>(re)[2 * e + 1] = (int8_t)o_im;
    return (int)c_re + (int)c_im;
}

} // namespace

GAT_API int32_t gat_condition_samples(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const gat_cond_params *params, uint32_t flags,
                                      const gat_signal_desc *out, uint64_t *counts)
{
    if (!c) return GAT_ERR_ARG;
    CondPlan plan{};
    const Refusal r = cond_plan(sig, B, params, flags, out, (long long)c->num_cus * 8, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_condition_samples");
    CondArgs a{};
    a.re = sig->re;
    a.im = sig->im;
    a.out_re = const_cast<void *>(out->re);
    a.out_im = const_cast<void *>(out->im);
    a.M = sig->num_ants;
    a.blank_all = (flags & GAT_COND_BLANK_ALL_ANTS) ? 1 : 0;
    a.N = sig->num_samples;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.out_ant_stride = out->ant_stride;
    a.out_block_stride = out->block_stride;
    a.chunk = plan.chunk;
    a.chunks = plan.chunks;
    a.units = plan.units;
    a.counts = reinterpret_cast<unsigned long long *>(counts);
    GAT_HIP(c, plan.stream ? launch_cond_stream(a, sig->layout, out->layout, params, (int)plan.grid, c->stream)
                           : launch_cond_general(a, sig->layout, out->layout, params, (int)plan.grid, c->stream));
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)plan.grid;
    c->last.threads = kCondThreads;
    c->last.splits = (int32_t)plan.chunks;
    c->last.ant_tile = a.M;
    c->last.vec = plan.stream ? 4 : 1;
    // the general kernel's records and counters in LDS; the streaming kernel keeps both in registers
    c->last.lds_bytes = plan.stream ? 0 : (int32_t)(GAT_MAX_ARRAY_ANTS * (sizeof(float4) + 2 * sizeof(unsigned long long)));
    return GAT_OK;
}

GAT_API int32_t gat_condition_samples_host(const gat_signal_desc *sig, int32_t B, const gat_cond_params *params, uint32_t flags,
                                           const gat_signal_desc *out, uint64_t *counts)
{
    CondPlan plan{};
    const Refusal r = cond_plan(sig, B, params, flags, out, 1, &plan);
    if (r.code != GAT_OK) return r.code;
    const int M = sig->num_ants;
    const bool blank_all = (flags & GAT_COND_BLANK_ALL_ANTS) != 0;
    float xr[GAT_MAX_ARRAY_ANTS], xi[GAT_MAX_ARRAY_ANTS];
    for (int b = 0; b < B; ++b)
        for (int64_t n = 0; n < sig->num_samples; ++n) {
            bool any = false;
            for (int m = 0; m < M; ++m) { // every antenna is read before any is written: in place is safe
                host_load_sample(sig, (size_t)n + (size_t)m * (size_t)sig->ant_stride + (size_t)b * (size_t)sig->block_stride, &xr[m], &xi[m]);
                any |= !cond_keep(xr[m], xi[m], params[m].threshold);
            }
            for (int m = 0; m < M; ++m) {
                const bool blanked = blank_all ? any : !cond_keep(xr[m], xi[m], params[m].threshold);
                const int clips = host_store(out, (size_t)n + (size_t)m * (size_t)out->ant_stride + (size_t)b * (size_t)out->block_stride, !blanked,
                                             xr[m], xi[m], params[m]);
                if (counts) counts[2 * m] += blanked ? 1u : 0u, counts[2 * m + 1] += (uint64_t)clips;
            }
        }
    return GAT_OK;
}

GAT_API int32_t gat_sample_stats(gat_ctx *c, const gat_signal_desc *sig, int32_t B, int32_t bpe, const gat_cond_params *params, uint32_t flags,
                                 gat_sample_stats_t *stats)
{
    if (!c) return GAT_ERR_ARG;
    StatsPlan plan{};
    const Refusal r = stats_plan(sig, B, bpe, flags, stats, c->num_cus, &plan);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    GAT_ENTER(c, "gat_sample_stats");
    const int M = sig->num_ants;
    long long grid_all = 0, splits_all = 1;
    const int32_t rc = enqueue_estimates<StatsArgs>(c, sig, plan.est, [&](StatsArgs a, const EstimateLaunches &t) -> int32_t {
        a.blank_all = (flags & GAT_COND_BLANK_ALL_ANTS) ? 1 : 0;
        a.prm = params;
        a.partial = reinterpret_cast<gat_sample_stats_t *>(c->d_partial);
        GAT_HIP(c, launch_stats(a, sig->layout, plan.vec, c->stream));
        GAT_HIP(c, launch_stats_finish(a.partial, M, t.en, (int)t.G, stats + (size_t)t.e0 * M, c->stream));
        // gat_last_launch_info describes the whole call: the workgroups of every batch, the largest split
        grid_all += (long long)t.en * t.G * plan.tiles;
        splits_all = std::max(splits_all, t.splits);
        return GAT_OK;
    });
    if (rc != GAT_OK) return rc;
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)std::min<long long>(grid_all, 0x7fffffff);
    c->last.threads = kStatsThreads;
    c->last.splits = (int32_t)splits_all;
    c->last.ant_tile = plan.ant_tile;
    c->last.vec = plan.vec ? 4 : 1;
    c->last.lds_bytes = (int32_t)((kStatsThreads / 64) * plan.ant_tile * sizeof(gat_sample_stats_t));
    c->last.finalize_launched = 1;
    return GAT_OK;
}

GAT_API int32_t gat_agc_update(gat_ctx *c, const gat_sample_stats_t *stats, int32_t M, const gat_agc_config *cfg, gat_cond_params *params)
{
    if (!c) return GAT_ERR_ARG;
    if (!stats || !params || !cfg) return fail(c, GAT_ERR_ARG, "null argument");
    if (M < 1) return fail(c, GAT_ERR_ARG, "num_ants must be positive");
    if (M > GAT_MAX_ARRAY_ANTS) return fail(c, GAT_ERR_RANGE, "more than 64 antennas");
    if (!agc_config_ok(cfg)) return fail(c, GAT_ERR_ARG, "bad AGC configuration");
    GAT_ENTER(c, "gat_agc_update");
    GAT_HIP(c, launch_agc_update(stats, M, cfg->target_rms, cfg->blank_factor, cfg->remove_dc, params, c->stream));
    return GAT_OK;
}

GAT_API int32_t gat_agc_update_host(const gat_sample_stats_t *stats, int32_t M, const gat_agc_config *cfg, gat_cond_params *params)
{
    if (!stats || !params || !cfg || M < 1 || !agc_config_ok(cfg)) return GAT_ERR_ARG;
    if (M > GAT_MAX_ARRAY_ANTS) return GAT_ERR_RANGE;
    for (int m = 0; m < M; ++m) params[m] = agc_record(stats[m], cfg->target_rms, cfg->blank_factor, cfg->remove_dc);
    return GAT_OK;
}
