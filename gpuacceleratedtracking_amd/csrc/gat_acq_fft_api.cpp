// gat_acq_fft_api.cpp -- host side of the FFT acquisition search (include/gat.h gat_acquire_fft, gat_acquire_fft_plan,
// gat_acquire_fft_host): the launch sequence behind the pure plan of gat_acq_fft_plan.h -- {twiddles; per unit batch: replica
// spectra; per Doppler batch: signal spectra; per step: products into the grid}, inside the frame both searches share
// (gat_acq_frame.h: its tail is {group sum, statistics} of gat_acq.hip) -- and the host twin, which runs the loops of gat_acq_fft.h.
// The kernels are gat_acq_fft.hip.
#include <algorithm>

#include "gat_acq_fft.h"
#include "gat_acq_fft_kernels.h"
#include "gat_acq_frame.h"

using namespace gat;

GAT_API int32_t gat_acquire_fft_plan(const gat_signal_desc *sig, int32_t B, int32_t P, double fs, const gat_acq_config *cfg, int32_t fft_log2,
                                     int32_t doppler_batch, int32_t unit_batch, int32_t num_cus, int32_t own_power, gat_acq_fft_plan *out)
{
    if (!out || out->struct_size < sizeof(gat_acq_fft_plan)) return GAT_ERR_ARG;
    AcqFftPlan plan{};
    const Refusal r = acq_fft_plan(sig, B, P, fs, cfg, AcqFftOptions{fft_log2, doppler_batch, unit_batch, 0}, num_cus, own_power != 0, &plan);
    if (r.code != GAT_OK) return r.code;
    acq_fft_report(plan, out);
    return GAT_OK;
}

GAT_API int32_t gat_acquire_fft_host(const gat_signal_desc *sig, int32_t B, const int8_t *codes, int32_t code_length, int32_t code_row_stride,
                                     const int32_t *prns, int32_t P, double fs, const gat_acq_config *cfg_in, int32_t fft_log2, int32_t unit_groups,
                                     float *power)
{
    if (!sig || !codes || !prns || !cfg_in || !power) return GAT_ERR_ARG;
    if (code_length < 1 || code_row_stride < code_length || unit_groups < 1 || fft_log2 == 0) return GAT_ERR_ARG;
    if (cfg_in->struct_size < sizeof(gat_acq_config)) return GAT_ERR_ARG;
    gat_acq_config cfg = *cfg_in;
    cfg.struct_size = sizeof(gat_acq_config);
    if (cfg.code_length == 0) cfg.code_length = code_length;
    if (cfg.code_length != code_length) return GAT_ERR_ARG;
    AcqFftPlan plan{};
    const Refusal r = acq_fft_plan(sig, B, P, fs, &cfg, AcqFftOptions{fft_log2, 0, 0, unit_groups}, 1, false, &plan);
    if (r.code != GAT_OK) return r.code;
    for (int p = 0; p < P; ++p)
        if (prns[p] < 0) return GAT_ERR_RANGE;
    acq_fft_host_run(sig, codes, code_row_stride, prns, fs, cfg, plan, power);
    return GAT_OK;
}

GAT_API int32_t gat_acquire_fft(gat_ctx *c, const gat_signal_desc *sig, int32_t B, const int32_t *prns, int32_t P, double fs,
                                const gat_acq_config *cfg_in, float *power_dev, gat_acq_result *res)
{
    gat_acq_config cfg;
    int32_t rc = acq_check_entry(c, sig, B, prns, P, fs, cfg_in, res, &cfg);
    if (rc != GAT_OK) return rc;
    AcqFftPlan pl{};
    const Refusal r = acq_fft_plan(sig, B, P, fs, &cfg, AcqFftOptions{c->acq_fft_log2, c->acq_fft_dbatch, c->acq_fft_ubatch, 0}, c->num_cus,
                                   power_dev == nullptr, &pl);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    rc = acq_run<AcqFftArgs>(c, "gat_acquire_fft", sig, B, prns, P, fs, cfg, pl, pl.Gu, power_dev, res, [&](AcqFftArgs &a, unsigned char *scr) -> int32_t {
        a.L = pl.L, a.L1 = pl.L1, a.L2 = pl.L2, a.tiles = pl.tiles, a.G = pl.G, a.Db = pl.Db, a.Gu = pl.Gu, a.Bb = pl.Bb;
        a.Jseg = pl.Jseg, a.units = pl.units, a.cells = (long long)P * pl.D * pl.J;
        a.scale = acq_fft_scale(pl.L);
        a.tw = reinterpret_cast<float2 *>(scr + pl.off_tw);
        a.C = reinterpret_cast<float2 *>(scr + pl.off_C);
        a.W = reinterpret_cast<float2 *>(scr + pl.off_W);
        a.Y = pl.passes == 2 ? reinterpret_cast<float2 *>(scr + pl.off_Y) : nullptr;
        GAT_HIP(c, launch_acq_fft_twiddles(a, c->stream));
        for (long long ub = 0; ub < pl.units; ub += pl.Ub) {
            a.u0 = (int)ub;
            a.un = (int)std::min<long long>(pl.Ub, pl.units - ub);
            a.b0 = a.u0 / pl.M;
            a.bn = (a.u0 + a.un - 1) / pl.M - a.b0 + 1;
            a.i0 = 0, a.dn = std::min(pl.Db, pl.D);
            GAT_HIP(c, launch_acq_fft_replica(a, c->stream));
            for (int i0 = 0; i0 < pl.D; i0 += pl.Db) {
                a.i0 = i0;
                a.dn = std::min(pl.Db, pl.D - i0);
                GAT_HIP(c, launch_acq_fft_signal(a, sig->layout, c->stream));
                for (int us = a.u0; us < a.u0 + a.un; us += pl.Gu) {
                    a.us = us;
                    GAT_HIP(c, launch_acq_fft_correlate(a, c->stream));
                }
            }
        }
        return GAT_OK;
    });
    if (rc != GAT_OK) return rc;
    c->last = gat_launch_info{};
    c->last.workgroups = (int32_t)std::min<long long>((long long)pl.Gu * P * pl.Db * pl.G * pl.tiles, 2147483647ll);
    c->last.threads = kAcqFftThreads;
    c->last.splits = pl.Gu;
    c->last.ant_tile = 1;
    c->last.vec = 1;
    c->last.lds_bytes = (1 << kAcqFftTileLog2) * 2 * (int)sizeof(float);
    c->last.channels_per_wg = 1;
    return GAT_OK;
}
