// gat_sample_load.h -- how the kernels over the raw sample stream (gat_fir.hip, gat_spec.hip) read a gat_signal_desc's memory: one
// sample with scalar loads, or the samples of one 16-byte load per plane.  Integer layouts convert exactly.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

#include "gat.h"
#include "gat_sig_plan.h"

namespace gat {

typedef unsigned u4 __attribute__((ext_vector_type(4)));

template <int FMT>
__device__ __forceinline__ void fir_load_scalar(const void *re, const void *im, size_t e, float &xr, float &xi)
{
    if constexpr (FMT == GAT_LAYOUT_PLANAR) {
        xr = static_cast<const float *>(re)[e];
        xi = static_cast<const float *>(im)[e];
    } else if constexpr (FMT == GAT_LAYOUT_INTERLEAVED) {
        xr = static_cast<const float *>(re)[2 * e];
        xi = static_cast<const float *>(re)[2 * e + 1];
    } else if constexpr (FMT == GAT_LAYOUT_INTERLEAVED_I16) {
        xr = (float)static_cast<const short *>(re)[2 * e];
        xi = (float)static_cast<const short *>(re)[2 * e + 1];
    } else {
        xr = (float)static_cast<const signed char *>(re)[2 * e];
        xi = (float)static_cast<const signed char *>(re)[2 * e + 1];
    }
}

// one 16-byte load per plane: VS samples
template <int FMT>
struct FirVec {
    static constexpr int VS = layout_vec_samples(FMT);
    u4 a, b; // b: the imaginary plane's 16 bytes (planar only)

    // vector v (VS samples) of the antenna stream that starts `base` samples into the planes, on a 16-byte boundary
    __device__ __forceinline__ void load(const void *re, const void *im, size_t base, long long v)
    {
        constexpr size_t sample_bytes = layout_sample_bytes(FMT);
        a = *(reinterpret_cast<const u4 *>(static_cast<const char *>(re) + base * sample_bytes) + v);
        if constexpr (FMT == GAT_LAYOUT_PLANAR) b = *(reinterpret_cast<const u4 *>(static_cast<const char *>(im) + base * sample_bytes) + v);
    }
    __device__ __forceinline__ float2 sample(int s) const
    {
        if constexpr (FMT == GAT_LAYOUT_PLANAR) {
            return make_float2(__uint_as_float(a[s]), __uint_as_float(b[s]));
        } else if constexpr (FMT == GAT_LAYOUT_INTERLEAVED) {
            return make_float2(__uint_as_float(a[2 * s]), __uint_as_float(a[2 * s + 1]));
        } else if constexpr (FMT == GAT_LAYOUT_INTERLEAVED_I16) {
            const unsigned w = a[s]; // (shifted left as unsigned, right as signed: the sign extension)
            return make_float2((float)((int)(w << 16) >> 16), (float)((int)w >> 16));
        } else {
            const unsigned w = a[s / 2];
            return make_float2((float)((int)(w << (24 - 16 * (s % 2))) >> 24), (float)((int)(w << (16 - 16 * (s % 2))) >> 24));
        }
    }
};

} // namespace gat
