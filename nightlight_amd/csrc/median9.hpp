// median9.hpp -- the 19-step median-of-9 exchange network (median3x3.go:85-110), shared by the
// 3x3 median filter (frame_stats.hip) and the bad-pixel replacement (preprocess.hip).  min / max
// only, so the result is bit-exact for NaN-free input.  Operands in the reference's gather order:
// row above, own row, row below, each left to right.
#pragma once
#include <hip/hip_runtime.h>

namespace nl {

#define NL_CE(i, j) { const float lo_ = fminf(a##i, a##j); a##j = fmaxf(a##i, a##j); a##i = lo_; }
#define NL_MAXTO(i, j) { a##j = fmaxf(a##i, a##j); }
#define NL_MINTO(i, j) { a##i = fminf(a##i, a##j); }

__device__ __forceinline__ float median9(float a0, float a1, float a2, float a3, float a4, float a5,
                                         float a6, float a7, float a8)
{
    NL_CE(0, 1) NL_CE(3, 4) NL_CE(6, 7)
    NL_CE(1, 2) NL_CE(4, 5) NL_CE(7, 8)
    NL_CE(0, 1) NL_CE(3, 4) NL_CE(6, 7)
    NL_MAXTO(0, 3)
    NL_MAXTO(3, 6)
    NL_CE(1, 4)
    NL_MINTO(4, 7)
    NL_MAXTO(1, 4)
    NL_MINTO(5, 8)
    NL_MINTO(2, 5)
    NL_CE(2, 4)
    NL_MINTO(4, 6)
    NL_MAXTO(2, 4)
    return a4;
}

#undef NL_CE
#undef NL_MAXTO
#undef NL_MINTO

// The same network with the reference's own steps, `if a[i] > a[j] { ... }` (median3x3.go:85-110): also exact where a
// NaN or a +0 / -0 tie takes part (a false comparison leaves both in place; fminf / fmaxf would pick one).
#define NL_CE(i, j) { const bool g_ = a##i > a##j; const float lo_ = g_ ? a##j : a##i; a##j = g_ ? a##i : a##j; a##i = lo_; }
#define NL_MAXTO(i, j) { if (a##i > a##j) a##j = a##i; }
#define NL_MINTO(i, j) { if (a##i > a##j) a##i = a##j; }

__device__ __forceinline__ float median9_cmp(float a0, float a1, float a2, float a3, float a4, float a5,
                                             float a6, float a7, float a8)
{
    NL_CE(0, 1) NL_CE(3, 4) NL_CE(6, 7)
    NL_CE(1, 2) NL_CE(4, 5) NL_CE(7, 8)
    NL_CE(0, 1) NL_CE(3, 4) NL_CE(6, 7)
    NL_MAXTO(0, 3)
    NL_MAXTO(3, 6)
    NL_CE(1, 4)
    NL_MINTO(4, 7)
    NL_MAXTO(1, 4)
    NL_MINTO(5, 8)
    NL_MINTO(2, 5)
    NL_CE(2, 4)
    NL_MINTO(4, 6)
    NL_MAXTO(2, 4)
    return a4;
}

#undef NL_CE
#undef NL_MAXTO
#undef NL_MINTO

// median9_cmp on a buffer, in place, as MedianFloat32Slice9 leaves it (median3x3.go:85-110): GatherAndMedian
// (gather.go:26-38) reuses one 9-slot buffer, so where a mask leaves the data the slots it does not fill keep what the
// network left there for the previous call (star detection's bad-pixel test, stars.hip).
#define NL_CE(i, j) { const bool g_ = a[i] > a[j]; const float lo_ = g_ ? a[j] : a[i]; a[j] = g_ ? a[i] : a[j]; a[i] = lo_; }
#define NL_MAXTO(i, j) { if (a[i] > a[j]) a[j] = a[i]; }
#define NL_MINTO(i, j) { if (a[i] > a[j]) a[i] = a[j]; }

__host__ __device__ inline float median9_cmp_buf(float (&a)[9])
{
    NL_CE(0, 1) NL_CE(3, 4) NL_CE(6, 7)
    NL_CE(1, 2) NL_CE(4, 5) NL_CE(7, 8)
    NL_CE(0, 1) NL_CE(3, 4) NL_CE(6, 7)
    NL_MAXTO(0, 3)
    NL_MAXTO(3, 6)
    NL_CE(1, 4)
    NL_MINTO(4, 7)
    NL_MAXTO(1, 4)
    NL_MINTO(5, 8)
    NL_MINTO(2, 5)
    NL_CE(2, 4)
    NL_MINTO(4, 6)
    NL_MAXTO(2, 4)
    return a[4];
}

#undef NL_CE
#undef NL_MAXTO
#undef NL_MINTO

}  // namespace nl
