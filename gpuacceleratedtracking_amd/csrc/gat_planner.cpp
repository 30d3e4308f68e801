// gat_planner.cpp -- the correlator call (gat::correlate_impl) in three steps that do not overlap: validation of the call
// (corr_check_call), the launch plan -- kernel selection (vector / matrix-core), tiling, splits, LDS sizing -- as a value that
// touches neither the device nor the context (corr_plan; corr_plan_resident for the resident correlator), both in the pure
// header gat_corr_plan.h, and its enqueue here (enqueue_plan: scratch, uploads, completion flags, the launches, the launch info).
#include <algorithm>
#include <cstring>

#include "gat_ctx.h"

using namespace gat;

namespace {

int32_t enqueue_plan(gat_ctx *c, const CorrCall &call, CorrPlan &p)
{
    const int B = call.B, K = call.K, L = call.L, M = call.sig->num_ants;
    if (p.kind && !p.m.params) {
        const int32_t rc = upload_params(c, call.params_inline, (size_t)B * K);
        if (rc != GAT_OK) return rc;
        p.m.params = c->d_params;
    }
    if (call.flags & GAT_FLAG_ATOMIC) {
        const size_t out_elems = (size_t)B * K * L * M;
        GAT_HIP(c, hipMemsetAsync(call.out_re, 0, out_elems * sizeof(float), c->stream));
        GAT_HIP(c, hipMemsetAsync(call.out_im, 0, out_elems * sizeof(float), c->stream));
    } else if (p.splits > 1) {
        const int32_t rc = ensure_partial(c, (size_t)B * K * p.splits * L * M * 2 * sizeof(float));
        if (rc != GAT_OK) return rc;
    }
    if (p.kind) {
        p.m.partial = c->d_partial;
        if (p.kind == 2)
            GAT_HIP(c, launch_mfma_bf16(p.m, p.rt, p.nct, call.sig->layout, p.grid, p.lds, c->stream));
        else
            GAT_HIP(c, launch_mfma(p.m, p.nct, p.grid, p.lds, c->stream));
        if (p.finalize) GAT_HIP(c, launch_finalize(c->d_partial, call.out_re, call.out_im, p.splits, L * M * 2, (long long)B * K, c->stream));
        c->last = p.info;
        return GAT_OK;
    }

    // completion flag: small launches outside a stream capture (a replayed graph would store a stale number)
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    (void)hipStreamIsCapturing(c->stream, &cap);
    // (library-owned streams only: nobody else can have enqueued newer work on them behind the library's back)
    const bool flagged = c->own_stream && c->d_flag && c->flag_max_wgs > 0 && (long long)p.a[0].total_wgs <= c->flag_max_wgs && cap == hipStreamCaptureStatusNone;
    (void)hipGetLastError();
    auto next_seq = [&]() { // sequence numbers of flagged launches: never 0 (0 = "nothing to wait for")
        if (++c->flag_seq == 0) ++c->flag_seq;
        return c->flag_seq;
    };
    for (int g = 0; g < p.groups; ++g) {
        DcArgs &a = p.a[g];
        a.partial = c->d_partial;
        // completion flag: carried by the call's last launch -- the last tap group's kernel, or the second stage behind it
        if (flagged && !p.finalize && !p.tail && g == p.groups - 1) {
            a.done_counter = c->d_done;
            a.host_flag = c->d_flag;
            a.flag_seq = next_seq();
        }
        GAT_HIP(c, launch_dc(a, p.cfg[g], c->stream));
    }
    if (p.finalize) {
        const bool carry = flagged && !p.tail;
        GAT_HIP(c, launch_finalize(c->d_partial, call.out_re, call.out_im, p.splits, L * M * 2, (long long)B * K, c->stream,
                                   carry ? c->d_done : nullptr, c->d_flag, carry ? next_seq() : 0u));
    }
    if (p.tail) {
        const DcArgs &a = p.a[0];
        DcTailArgs tl{a.re, a.im, a.params, a.codes, a.out_re, a.out_im, nullptr, nullptr, 0u, a.N, a.ant_stride, a.block_stride, a.chan_stride, a.fs,
                      a.M, a.K, a.B, a.Ltot, a.Lc, a.num_prns, a.code_row_stride, call.sig->layout, a.n_vec, a.max_abs_shift, {}, {}};
        std::copy(call.shifts, call.shifts + L, tl.shifts);
        std::memcpy(tl.inl, a.inl, sizeof tl.inl);
        if (flagged) {
            tl.done_counter = c->d_done;
            tl.host_flag = c->d_flag;
            tl.flag_seq = next_seq();
        }
        GAT_HIP(c, launch_dc_tail(tl, c->stream));
    }
    if (flagged) c->wait_seq = c->flag_seq;
    c->last = p.info;
    return GAT_OK;
}

} // namespace

// (declared in gat_ctx.h)
int32_t gat::correlate_impl(gat_ctx *c, const gat_signal_desc *sig, const gat_channel_params *params_dev,
                            int32_t B, int32_t K, int32_t L, const int32_t *shifts, double fs,
                            float *out_re, float *out_im, uint32_t flags, const gat_channel_params *params_inline)
{
    // (not the entry preamble of gat_ctx.h: every caller arrives here after its own hipSetDevice, the loop once per block)
    c->wait_seq = 0;
    const TraceRange trace("gat_downconvert_and_correlate");
    if (!sig || (!params_dev && !params_inline) || !shifts || !out_re || !out_im) return fail(c, GAT_ERR_ARG, "null argument");
    const CorrCall call{sig, params_dev, params_inline, B, K, L, shifts, fs, out_re, out_im, flags};
    const CorrTables tables = corr_tables(*c);
    Refusal r = corr_check_call(tables, call);
    CorrPlan p;
    if (r.code == GAT_OK) r = corr_plan(c->knobs, tables, call, p);
    if (r.code != GAT_OK) return fail(c, r.code, r.msg);
    return enqueue_plan(c, call, p);
}
