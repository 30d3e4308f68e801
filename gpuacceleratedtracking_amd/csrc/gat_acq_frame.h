// gat_acq_frame.h -- what the two acquisition entry points (gat_acquire: gat_acq_api.cpp, gat_acquire_fft: gat_acq_fft_api.cpp)
// do alike around their own launches, stated once: the checks before planning, the arguments both kernels' families take, and the
// frame {enter, scratch, PRN upload; the search's launches; group sum, statistics, result copy, sync}.  Header-only: the two
// entry points are translation units of their own and only the first belongs to the host simulator (tests/hostsim).
#pragma once

#include "gat_acq_kernels.h"
#include "gat_acq_plan.h"
#include "gat_ctx.h"

namespace gat {

// What needs the context, then the call check of gat_acq_plan.h against the bound code table; *cfg: the normalised configuration.
inline int32_t acq_check_entry(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const int32_t *prns, int32_t P, double fs,
                               const gat_acq_config *cfg_in, const gat_acq_result *res, gat_acq_config *cfg)
{
    if (!c) return GAT_ERR_ARG;
    if (!sig || !prns || !res) return fail(c, GAT_ERR_ARG, "null argument");
    if (!c->d_codes) return fail(c, GAT_ERR_STATE, "gat_set_codes has not been called");
    const Refusal r = acq_check_call(cfg_in, B, prns, P, fs, c->Lc, c->P, cfg);
    return r.code == GAT_OK ? GAT_OK : fail(c, r.code, r.msg);
}

// the fields AcqArgs and AcqFftArgs both have; the groups and the rest of the plan are each search's own
template <class Args>
Args acq_args(const gat_ctx *c, const gat_signal_desc *sig, int32_t B, int32_t P, double fs, const gat_acq_config &cfg, const int *d_prns, float *out)
{
    Args a{};
    a.re = sig->re;
    a.im = sig->im;
    a.M = sig->num_ants;
    a.B = B;
    a.N = sig->num_samples;
    a.ant_stride = sig->ant_stride;
    a.block_stride = sig->block_stride;
    a.codes = c->d_codes;
    a.code_row_stride = c->code_row_stride;
    a.Lc = c->Lc;
    a.prns = d_prns;
    a.P = P;
    a.D = cfg.num_doppler_bins;
    a.J = cfg.num_code_bins;
    a.s = cfg.code_step_samples;
    a.ratio = cfg.code_freq_hz / fs;
    a.fs = fs;
    a.if_hz = cfg.if_hz;
    a.f_first = cfg.doppler_first_hz;
    a.f_step = cfg.doppler_step_hz;
    a.first_shift = cfg.first_shift;
    a.out = out;
    return a;
}

// A planned search on the context's stream.  scr: the plan's regions in c->d_partial; groups: the unit groups whose slices the
// tail adds (1: the launches write the power grid itself).  search(a, base) enqueues the search's own launches on the common
// arguments a -- a.out is where they put their sums -- with base the start of the scratch, for the plan's other regions; what it
// returns but GAT_OK ends the call.  The trace range `range` opens here and so covers the launches.
template <class Args, class Search>
int32_t acq_run(gat_ctx *c, const char *range, const gat_signal_desc *sig, int32_t B, const int32_t *prns, int32_t P, double fs,
                const gat_acq_config &cfg, const AcqScratch &scr, int groups, float *power_dev, gat_acq_result *res, Search &&search)
{
    GAT_ENTER(c, range);
    {
        const int32_t rc = ensure_partial(c, scr.bytes);
        if (rc != GAT_OK) return rc;
    }
    unsigned char *base = reinterpret_cast<unsigned char *>(c->d_partial);
    int *d_prns = reinterpret_cast<int *>(base + scr.off_prn);
    gat_acq_result *d_res = reinterpret_cast<gat_acq_result *>(base + scr.off_res);
    float *power = power_dev ? power_dev : reinterpret_cast<float *>(base + scr.off_pow);
    GAT_HIP(c, hipMemcpyAsync(d_prns, prns, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));

    Args a = acq_args<Args>(c, sig, B, P, fs, cfg, d_prns, groups > 1 ? reinterpret_cast<float *>(base + scr.off_part) : power);
    {
        const int32_t rc = search(a, base);
        if (rc != GAT_OK) return rc;
    }
    if (groups > 1) GAT_HIP(c, launch_acq_sum_groups(a.out, power, (long long)P * a.D * a.J, groups, c->stream));
    GAT_HIP(c, launch_acq_stats(power, P, a.D, a.J, cfg, fs, a.N, d_prns, d_res, c->stream));
    GAT_HIP(c, hipMemcpyAsync(res, d_res, (size_t)P * sizeof(gat_acq_result), hipMemcpyDeviceToHost, c->stream));
    GAT_HIP(c, hipStreamSynchronize(c->stream));
    return GAT_OK;
}

} // namespace gat
