// gat_eig.hip -- the subspace kernels (include/gat.h gat_accumulator_covariance, gat_hermitian_eig) for gfx950.  The arithmetic is
// gat_eig.h (the host twins run the same text), the geometry and the decoding of a work unit gat_eig_plan.h.  Every value meets
// the same operands in the same order whichever lane holds it: no atomics, no reduction tree, no data-dependent order.
#include "gat_eig_kernels.h"

namespace gat {

namespace {

// ---- accumulator covariance ------------------------------------------------------------------------------------------------------
// The entries of one thread: t = thread, thread + kCovThreads, ... < T, each with its (i, j) and its running sums.
struct CovEntries {
    double re[kCovEntriesPerThread], im[kCovEntriesPerThread];
    int i[kCovEntriesPerThread], j[kCovEntriesPerThread];
};

__device__ inline void cov_entries_begin(CovEntries &s, int T)
{
#pragma unroll
    for (int v = 0; v < kCovEntriesPerThread; ++v) {
        const int t = v * kCovThreads + (int)threadIdx.x;
        s.i[v] = s.j[v] = 0;
        if (t < T) cov_entry(t, &s.i[v], &s.j[v]);
    }
}

// The sums of the blocks first .. first + count of channel k, from +0 in block order.  The workgroup stages kCovPiece blocks'
// M-vectors in LDS at a time -- consecutive threads load consecutive antennas of a block, as the monitor's prompt kernel reads
// them --, then every thread walks the staged blocks in order for its entries.  first and count are the workgroup's: the barriers
// are uniform.
__device__ inline void cov_walk(const AccCovArgs &a, int k, int first, int count, float *s_re, float *s_im, CovEntries &s)
{
    const int M = a.M, T = a.T, tid = (int)threadIdx.x;
#pragma unroll
    for (int v = 0; v < kCovEntriesPerThread; ++v) s.re[v] = s.im[v] = 0.0;
    const size_t tap = ((size_t)k * a.L + a.tap) * M;
    for (int c0 = 0; c0 < count; c0 += kCovPiece) {
        const int nb = count - c0 < kCovPiece ? count - c0 : kCovPiece;
        __syncthreads(); // the piece before has been read
        for (int x = tid; x < nb * M; x += kCovThreads) {
            const int b = x / M, m = x % M;
            const size_t o = (size_t)(first + c0 + b) * (size_t)a.acc_block_stride + tap + m;
            s_re[x] = a.acc_re[o];
            s_im[x] = a.acc_im[o];
        }
        __syncthreads();
        for (int b = 0; b < nb; ++b) {
            const float *xr = s_re + b * M, *xi = s_im + b * M;
#pragma unroll
            for (int v = 0; v < kCovEntriesPerThread; ++v)
                if (v * kCovThreads + tid < T) cov_add(xr[s.i[v]], xi[s.i[v]], xr[s.j[v]], xi[s.j[v]], s.re[v], s.im[v]);
        }
    }
}

// entry (i, j) and its conjugate of estimate-and-channel ek
__device__ inline void cov_store(const AccCovArgs &a, long long ek, int i, int j, double re, double im)
{
    double *out_re = a.cov_re + (size_t)ek * a.M * a.M, *out_im = a.cov_im + (size_t)ek * a.M * a.M;
    if (i == j) im = 0.0;
    out_re[i * a.M + j] = re, out_im[i * a.M + j] = im;
    if (i != j) out_re[j * a.M + i] = re, out_im[j * a.M + i] = -im;
}

// one workgroup per (estimate, channel): its chunks in order, the chunk sums added from +0
__global__ __launch_bounds__(kCovThreads) void acc_cov_direct_kernel(AccCovArgs a)
{
    extern __shared__ __align__(16) unsigned char cov_lds[];
    float *s_re = reinterpret_cast<float *>(cov_lds), *s_im = s_re + kCovPiece * a.M;
    int e, k;
    if (!cov_direct_unit(blockIdx.x, a.E, a.K, &e, &k)) return;
    int b0, n;
    cov_estimate(e, a.bpe, a.B, &b0, &n);
    CovEntries s;
    cov_entries_begin(s, a.T);
    double tr[kCovEntriesPerThread], ti[kCovEntriesPerThread];
#pragma unroll
    for (int v = 0; v < kCovEntriesPerThread; ++v) tr[v] = ti[v] = 0.0;
    for (int c = 0; c < cov_chunks(n); ++c) {
        int first, count;
        cov_chunk(c, b0, n, &first, &count);
        cov_walk(a, k, first, count, s_re, s_im, s);
#pragma unroll
        for (int v = 0; v < kCovEntriesPerThread; ++v) tr[v] += s.re[v], ti[v] += s.im[v];
    }
#pragma unroll
    for (int v = 0; v < kCovEntriesPerThread; ++v)
        if (v * kCovThreads + (int)threadIdx.x < a.T) cov_store(a, (long long)e * a.K + k, s.i[v], s.j[v], tr[v], ti[v]);
}

// one workgroup per (estimate, channel, chunk): the chunk's sums to the scratch
__global__ __launch_bounds__(kCovThreads) void acc_cov_chunk_kernel(AccCovArgs a)
{
    extern __shared__ __align__(16) unsigned char cov_lds[];
    float *s_re = reinterpret_cast<float *>(cov_lds), *s_im = s_re + kCovPiece * a.M;
    int e, k, c, b0, n, first, count;
    if (!cov_split_unit(blockIdx.x, a.E, a.K, a.C, &e, &k, &c)) return;
    cov_estimate(e, a.bpe, a.B, &b0, &n);
    if (!cov_chunk(c, b0, n, &first, &count)) return; // the last estimate is shorter: the whole workgroup leaves
    CovEntries s;
    cov_entries_begin(s, a.T);
    cov_walk(a, k, first, count, s_re, s_im, s);
    const size_t base = (size_t)blockIdx.x * a.T;
#pragma unroll
    for (int v = 0; v < kCovEntriesPerThread; ++v) {
        const int t = v * kCovThreads + (int)threadIdx.x;
        if (t < a.T) a.part_re[base + t] = s.re[v], a.part_im[base + t] = s.im[v];
    }
}

// one thread per (estimate, channel, entry): the chunk sums added in chunk order from +0
__global__ __launch_bounds__(kCovThreads) void acc_cov_reduce_kernel(AccCovArgs a)
{
    long long ek;
    int t, b0, n, i, j;
    if (!cov_reduce_unit((long long)blockIdx.x * kCovThreads + threadIdx.x, a.E, a.K, a.T, &ek, &t)) return;
    cov_estimate((int)(ek / a.K), a.bpe, a.B, &b0, &n);
    double tr = 0.0, ti = 0.0;
    for (int c = 0; c < cov_chunks(n); ++c) {
        const size_t o = ((size_t)ek * a.C + c) * a.T + t;
        tr += a.part_re[o], ti += a.part_im[o];
    }
    cov_entry(t, &i, &j);
    cov_store(a, ek, i, j, tr, ti);
}

// ---- Hermitian eigensolver -------------------------------------------------------------------------------------------------------
// One workgroup per matrix; A and V stay in LDS as FP64 planes (EigPlan says where).  A round: the first `pairs` threads compute
// the rotations from the same A; barrier; column phase, one item per (pair, row), on A and V; barrier; row phase, one item per
// (pair, column), on A; barrier.  Both phases update in place: an item owns the two elements it reads.  The sweep's flag is read
// by every thread after a barrier, so the data-dependent sweep count is the workgroup's and no thread leaves before the last one.
template <bool F32>
__global__ __launch_bounds__(kEigThreadsLarge) void hermitian_eig_kernel(EigArgs a)
{
    extern __shared__ __align__(16) unsigned char eig_lds[];
    const EigPlan &p = a.p;
    const int Q = p.Q, ld = p.ld, pairs = p.pairs, tid = (int)threadIdx.x, nt = (int)blockDim.x, mat = (int)blockIdx.x;
    double *base = reinterpret_cast<double *>(eig_lds);
    double *are = base, *aim = base + p.plane, *vre = base + p.off_vre, *vim = vre + p.plane; // V: only with want_vec
    double *s_c = base + p.off_rot, *s_gr = s_c + pairs, *s_gi = s_gr + pairs;
    double *s_d = base + p.off_col, *s_fr = s_d + Q, *s_fi = s_fr + Q, *s_mod = s_fi + Q;
    double *s_F = base + p.off_f;
    int *s_pq = reinterpret_cast<int *>(base + p.off_int), *s_rank = s_pq + pairs, *s_m = s_rank + Q, *s_any = s_m + Q;

    const size_t in0 = (size_t)mat * Q * Q;
    for (int x = tid; x < Q * Q; x += nt) {
        const int i = x / Q, j = x % Q;
        if (j > i) continue;
        double r, m;
        if (F32)
            r = (double)static_cast<const float *>(a.a_re)[in0 + x], m = (double)static_cast<const float *>(a.a_im)[in0 + x];
        else
            r = static_cast<const double *>(a.a_re)[in0 + x], m = static_cast<const double *>(a.a_im)[in0 + x];
        if (i == j) m = 0.0;
        are[i * ld + j] = r, aim[i * ld + j] = m;
        are[j * ld + i] = r, aim[j * ld + i] = -m;
    }
    if (p.want_vec)
        for (int x = tid; x < Q * Q; x += nt) {
            const int i = x / Q, j = x % Q;
            vre[i * ld + j] = i == j ? 1.0 : 0.0, vim[i * ld + j] = 0.0;
        }
    __syncthreads();
    if (tid == 0) { // F: one sum in row-major order
        double F = 0.0;
        for (int i = 0; i < Q; ++i)
            for (int j = 0; j < Q; ++j) F += are[i * ld + j] * are[i * ld + j] + aim[i * ld + j] * aim[i * ld + j];
        *s_F = F;
    }
    __syncthreads();
    const double F = *s_F;
    double *ev = a.eigenvalues ? a.eigenvalues + (size_t)mat * Q : nullptr;
    double *wr = p.want_vec ? a.vec_re + (size_t)mat * p.R * Q : nullptr, *wi = p.want_vec ? a.vec_im + (size_t)mat * p.R * Q : nullptr;
    if (!(F <= kEigFinite)) { // the whole workgroup: F is one value
        const double nan = __builtin_nan("");
        if (ev)
            for (int i = tid; i < Q; i += nt) ev[i] = nan;
        if (wr)
            for (int i = tid; i < p.R * Q; i += nt) wr[i] = wi[i] = nan;
        if (tid == 0 && a.status) a.status[mat] = -2;
        return;
    }
    const double limit = kEigThreshold * F;

    int sweeps = 0;
    bool converged = false;
    while (sweeps < GAT_EIG_MAX_SWEEPS) {
        if (tid == 0) *s_any = 0;
        __syncthreads();
        for (int r = 0; r < p.np - 1; ++r) {
            if (tid < pairs) {
                int pp = 0, qq = 0;
                const bool live = eig_pair(Q, r, tid, &pp, &qq) &&
                                  eig_rotation(are[pp * ld + pp], are[qq * ld + qq], are[pp * ld + qq], aim[pp * ld + qq], limit, &s_c[tid], &s_gr[tid], &s_gi[tid]);
                s_pq[tid] = live ? pp + 256 * qq : -1;
                if (live) *s_any = 1;
            }
            __syncthreads();
            for (int t = tid; t < pairs * Q; t += nt) {
                int s, row;
                eig_item(t, pairs, Q, &s, &row);
                const int pq = s_pq[s];
                if (pq < 0) continue;
                eig_col_item(are, aim, ld, row, pq % 256, pq / 256, s_c[s], s_gr[s], s_gi[s]);
                if (p.want_vec) eig_col_item(vre, vim, ld, row, pq % 256, pq / 256, s_c[s], s_gr[s], s_gi[s]);
            }
            __syncthreads();
            for (int t = tid; t < pairs * Q; t += nt) {
                int s, col;
                eig_item(t, pairs, Q, &s, &col);
                const int pq = s_pq[s];
                if (pq >= 0) eig_row_item(are, aim, ld, col, pq % 256, pq / 256, s_c[s], s_gr[s], s_gi[s]);
            }
            __syncthreads();
        }
        const int any = *s_any;
        __syncthreads(); // every thread has read the flag before the next sweep clears it
        if (!any) {
            converged = true;
            break;
        }
        ++sweeps;
    }

    if (tid < Q) s_d[tid] = are[tid * ld + tid];
    __syncthreads();
    if (tid < Q) {
        const int r = eig_rank(s_d, Q, tid);
        s_rank[tid] = r;
        if (ev) ev[r] = s_d[tid];
        if (p.want_vec && r < p.R) eig_phase(vre, vim, ld, Q, tid, &s_m[tid], &s_mod[tid], &s_fr[tid], &s_fi[tid]);
    }
    __syncthreads();
    if (p.want_vec)
        for (int x = tid; x < Q * Q; x += nt) {
            const int col = x / Q, row = x % Q, r = s_rank[col];
            if (r >= p.R) continue;
            eig_component(vre[row * ld + col], vim[row * ld + col], row == s_m[col], s_mod[col], s_fr[col], s_fi[col], &wr[(size_t)r * Q + row],
                          &wi[(size_t)r * Q + row]);
        }
    if (tid == 0 && a.status) a.status[mat] = converged ? sweeps : -1;
}

template <class Kernel>
hipError_t launch_cov(Kernel kernel, const AccCovArgs &a, long long grid, int lds, hipStream_t st)
{
    if (grid < 1 || grid > kEigMaxGrid) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(kCovThreads), lds, st, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_acc_cov_direct(const AccCovArgs &a, const AccCovPlan &p, hipStream_t st) { return launch_cov(acc_cov_direct_kernel, a, p.g_chunk, p.lds_bytes, st); }
hipError_t launch_acc_cov_chunks(const AccCovArgs &a, const AccCovPlan &p, hipStream_t st) { return launch_cov(acc_cov_chunk_kernel, a, p.g_chunk, p.lds_bytes, st); }
hipError_t launch_acc_cov_reduce(const AccCovArgs &a, const AccCovPlan &p, hipStream_t st) { return launch_cov(acc_cov_reduce_kernel, a, p.g_reduce, 0, st); }

hipError_t launch_hermitian_eig(const EigArgs &a, hipStream_t st)
{
    const EigPlan &p = a.p;
    if (p.g < 1 || p.g > kEigMaxGrid) return hipErrorInvalidValue;
    auto kernel = p.f32 ? hermitian_eig_kernel<true> : hermitian_eig_kernel<false>;
    // order 64 with vectors: four planes of 64 x 65 doubles = 130 KB; above 64 KB the function has to be told
    const hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, p.lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3((unsigned)p.g), dim3(p.threads), p.lds_bytes, st, a);
    return hipGetLastError();
}

} // namespace gat
