// gat_internal.h -- the kernel launchers that the C-ABI layer (gat_api.cpp, gat_planner.cpp, gat_resident_api.cpp) calls and the
// kernel files (gat_kernels.hip, gat_dc_f*.hip, gat_resident_f*.hip, gat_mfma*.hip) define.  What they are called WITH -- the
// argument structs and the constexpr geometry that host and kernels share -- is HIP-free and lives in gat_corr_plan.h.
#pragma once

#include <hip/hip_runtime.h>

#include "gat_corr_plan.h"

// The reduced instance set (-DGAT_DC_DEV) and the environment knobs of gat_create exist in development builds only
// (-DGAT_DEV); gat_version() names every flag of a build.
#if defined(GAT_DC_DEV) && !defined(GAT_DEV)
#error "-DGAT_DC_DEV needs -DGAT_DEV"
#endif

namespace gat {

// All return hipError_t of the launch.
hipError_t launch_dc(const DcArgs &a, const DcLaunch &cfg, hipStream_t s);
// one translation unit per sample format (gat_dc_f*.hip), so that the instances compile in parallel
template <int FMT> hipError_t launch_dc_fmt(const DcArgs &a, const DcLaunch &cfg, hipStream_t s);
hipError_t launch_dc_tail(const DcTailArgs &a, hipStream_t s);
// the resident correlator (gat_resident.h)
hipError_t launch_dc_resident(const DcArgs &a, const DcLaunch &cfg, const ResidentArgs &r, hipStream_t s);
// workgroups of the instance that one compute unit holds at once (occupancy API with the launch's LDS)
hipError_t dc_resident_blocks_per_cu(const DcLaunch &cfg, int *blocks_per_cu);
template <int FMT> hipError_t launch_dc_resident_fmt(const DcArgs &a, const DcLaunch &cfg, const ResidentArgs &r, hipStream_t s, int *blocks_per_cu);
hipError_t launch_mfma(const MfArgs &a, int nct, unsigned grid, unsigned lds_bytes, hipStream_t s);
// split-bf16 matrix-core kernel (gat_mfma_bf16.hip): rt = 16-antenna row tiles per workgroup (1, 2, 4)
hipError_t launch_mfma_bf16(const MfArgs &a, int rt, int nct, int fmt, unsigned grid, unsigned lds_bytes, hipStream_t s);
// done_counter != null: the launch ends by storing flag_seq into host_flag (completion flag, see gat_dc.h)
hipError_t launch_finalize(const float *partial, float *out_re, float *out_im, int splits, int elems,
                           long long groups, hipStream_t s, unsigned *done_counter = nullptr, unsigned *host_flag = nullptr,
                           unsigned flag_seq = 0);
hipError_t launch_gen_code_replica(float *rep, long long count, const int8_t *code_row, int Lc,
                                   double fc, double fs, double tau, long long first_shift,
                                   bool f32_coordinates, hipStream_t s);
// the texture-addressing study (gat.h gat_gen_code_replica_texaddr): fixed-point normalised coordinate / texel address
hipError_t launch_gen_code_replica_texaddr(float *rep, long long count, const int8_t *code_row, int Lc, double fc, double fs,
                                           double tau, long long first_shift, int coord_frac_bits, int texel_frac_bits,
                                           hipStream_t s);
// a kernel that only reads `bytes` (16-byte groups) of device memory (gat.h gat_debug_read_stream); sink: 4 bytes nobody reads
hipError_t launch_read_stream(const void *dev, size_t bytes, int variant, int num_cus, float *sink, hipStream_t s);
hipError_t launch_gen_code_replica_multi(float *rep, long long count, long long row_stride, int K,
                                         const gat_channel_params *params, const int8_t *codes, int code_row_stride,
                                         int Lc, int num_prns, double fs, long long first_shift, hipStream_t s);
hipError_t launch_accumulate_debug(const float *sig_re, const float *sig_im, long long N, int M, long long ant_stride,
                                   const gat_channel_params &P, const int8_t *code_row, int Lc, double fs, int L,
                                   const int *shifts_dev, float *car_re, float *car_im, float *dw_re, float *dw_im,
                                   float *acc_re, float *acc_im, hipStream_t s);
hipError_t launch_gen_signal(void *re, void *im, int format, long long N, int M,
                             long long ant_stride, long long block_stride, int B, int K,
                             const gat_channel_params *params, const int8_t *codes, int code_row_stride,
                             int Lc, int num_prns, double fs, float amplitude, const float *steering_cycles, float noise_sigma,
                             unsigned long long seed, hipStream_t s);
hipError_t launch_reduce_stage1(const float *in_re, const float *in_im, long long n, int cols,
                                int chunks, float *partial, hipStream_t s);
hipError_t launch_tracking_update(const float *acc_re, const float *acc_im, int K, int M, const gat_loop_config &cfg,
                                  gat_loop_state *state, const gat_channel_params *cur, gat_channel_params *next,
                                  hipStream_t s);

} // namespace gat
