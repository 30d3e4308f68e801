// gat_hd.h -- the one definition of the markers of text that host and device compile alike.  GAT_HD: a function of both builds
// (nothing for a plain C++ compiler).  GAT_HD_FORCEINLINE: the same, inlined wherever it is called (what __forceinline__ says
// on the device: the predicates of gat_chan_rules.h are part of the correlator kernels' text).  No HIP header.
#pragma once

#if defined(__HIPCC__)
#define GAT_HD __host__ __device__
#else
#define GAT_HD
#endif
#define GAT_HD_FORCEINLINE GAT_HD inline __attribute__((always_inline))
