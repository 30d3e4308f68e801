// gat_sample_load.h -- how every kernel over the raw sample stream (gat_acq.hip, gat_array.hip, gat_beam.hip, gat_cond.hip,
// gat_fir.hip, gat_spec.hip, gat_st.hip, gat_acq_fft.hip) reads a gat_signal_desc's memory: one sample with scalar loads, or the
// samples of one 16-byte load per plane.  Integer layouts convert exactly.  Device code only; the host's twin is
// host_load_sample (gat_sig_plan.h).  The correlator keeps a loader of its own (gat_dc.h SampleIO).
#pragma once

#include <hip/hip_runtime.h>

#include "gat.h"
#include "gat_sig_plan.h"

namespace gat {

typedef unsigned u4 __attribute__((ext_vector_type(4)));

// sample e of the planes
template <int FMT>
__device__ __forceinline__ void load_sample(const void *re, const void *im, size_t e, float &xr, float &xi)
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

// one 16-byte load per plane: VS samples.  NT: a non-temporal load, for a stream that is read once
template <int FMT, bool NT>
struct SampleVec {
    static constexpr int VS = layout_vec_samples(FMT);
    u4 a, b; // b: the imaginary plane's 16 bytes (planar only)

    static __device__ __forceinline__ u4 load16(const void *plane, size_t base, long long v)
    {
        const u4 *p = reinterpret_cast<const u4 *>(static_cast<const char *>(plane) + base * (size_t)layout_sample_bytes(FMT)) + v;
        if constexpr (NT)
            return __builtin_nontemporal_load(p);
        else
            return *p;
    }
    // vector v (VS samples) of the antenna stream that starts `base` samples into the planes, on a 16-byte boundary
    __device__ __forceinline__ void load(const void *re, const void *im, size_t base, long long v)
    {
        a = load16(re, base, v);
        if constexpr (FMT == GAT_LAYOUT_PLANAR) b = load16(im, base, v);
    }
    // sample s < VS: an int (a constant once the caller's loop is unrolled) or a std::integral_constant<int, s>.  The two are not
    // the same to the optimiser: it sees this function before it is inlined, and with an int it turns the 16-byte read into one
    // of a single element.  cov_small_kernel (gat_array.hip) was tuned on the constant's code and passes one; the others pass ints.
    template <class S>
    __device__ __forceinline__ void sample(S s_, float &xr, float &xi) const
    {
        const int s = s_;
        if constexpr (FMT == GAT_LAYOUT_PLANAR) {
            xr = __uint_as_float(a[s]);
            xi = __uint_as_float(b[s]);
        } else if constexpr (FMT == GAT_LAYOUT_INTERLEAVED) {
            xr = __uint_as_float(a[2 * s]);
            xi = __uint_as_float(a[2 * s + 1]);
        } else if constexpr (FMT == GAT_LAYOUT_INTERLEAVED_I16) {
            const unsigned w = a[s]; // (shifted left as unsigned, right as signed: the sign extension)
            xr = (float)((int)(w << 16) >> 16);
            xi = (float)((int)w >> 16);
        } else {
            const unsigned w = a[s / 2];
            xr = (float)((int)(w << (24 - 16 * (s % 2))) >> 24);
            xi = (float)((int)(w << (16 - 16 * (s % 2))) >> 24);
        }
    }
};

} // namespace gat
