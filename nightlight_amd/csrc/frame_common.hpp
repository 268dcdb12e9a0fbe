// frame_common.hpp -- what the kernels of the per-frame operators (preprocess.hip, bayer.hip, stars.hip,
// background.hip, frame_stats.hip, ingest.hip, tone.hip) share: the wave reductions, the block sum, Go's float -> int32; and,
// with the stack kernels (through wave_lists.hpp), Go's fp32 square root.
// Summation order is part of the results (fp64 partials feed bit-exact fp32 statistics): the butterfly runs over the
// xor distances 32, 16, ... 1, the wave values are added left to right.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nl {

// every lane gets the reduction over its wave of 64
template <class T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// number of lanes of a ballot below `lane`: a flagged lane's place among the wave's flagged lanes
__device__ __forceinline__ unsigned lane_rank(unsigned long long mask, int lane)
{
    return (unsigned)__popcll(mask & ((1ull << lane) - 1ull));
}
// (fminf / fmaxf: a NaN loses against a number)
__device__ __forceinline__ float wave_min(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_xor(v, off, 64));
    return v;
}

// The two halves of a block reduction: lane 0 of every wave puts its wave's value v into s[wave], then a barrier;
// s[0] + s[1] + ... + s[WAVES - 1] in that order.
template <class T>
__device__ __forceinline__ void wave_values(T v, T *s)
{
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
    __syncthreads();
}
template <int WAVES, class T>
__device__ __forceinline__ T sum_in_order(const T *s)
{
    T t = s[0];
#pragma unroll
    for (int w = 1; w < WAVES; w++) t += s[w];
    return t;
}

// the sum over a workgroup of THREADS = 64 k threads, in every thread; at most one call per kernel and T (the LDS is
// not fenced against a second one)
template <int THREADS, class T>
__device__ __forceinline__ T block_sum(T v)
{
    __shared__ T s[THREADS / 64];
    wave_values(wave_sum(v), s);
    return sum_in_order<THREADS / 64>(s);
}

// The end of a {min, sum, max} reduction over a workgroup of 256 (min_sum_max_kernel and the tone kernels that reduce
// what they write): the waves' butterflies, then wave 0's lane 0 folds the four wave values in order and writes the
// workgroup's partial[3 * blockIdx.x + {0, 1, 2}].  The statistics are bit-exact against the reference in this order.
__device__ __forceinline__ void block_min_sum_max(float mn, double sum, float mx, double *partial)
{
    __shared__ float s_mn[4], s_mx[4];
    __shared__ double s_sum[4];
    mn = wave_min(mn);
    mx = wave_max(mx);
    sum = wave_sum(sum);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mn[wave] = mn; s_mx[wave] = mx; s_sum[wave] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; w++) {
            mn = fminf(mn, s_mn[w]);
            mx = fmaxf(mx, s_mx[w]);
            sum += s_sum[w];
        }
        partial[3 * (size_t)blockIdx.x + 0] = (double)mn;
        partial[3 * (size_t)blockIdx.x + 1] = sum;
        partial[3 * (size_t)blockIdx.x + 2] = (double)mx;
    }
}

// Go's float32(math.Sqrt(float64(x))) (stats.go:259): the square root in fp64, rounded once to fp32 = the correctly
// rounded fp32 root.  NOT __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS HIP maps that to the 1-ulp native
// v_sqrt_f32, which flipped one clip decision in 2.1e9 samples against the oracle.
__device__ __forceinline__ float sqrt_go(float x)
{
    return (float)__builtin_sqrt((double)x);
}

// Go's float -> int32 conversion is CVTTSS2SL / CVTTSD2SL on amd64: truncation, and 0x80000000 for NaN or out of range
__host__ __device__ inline int32_t go_i32(float f)
{
    return (f >= -2147483648.0f && f < 2147483648.0f) ? (int32_t)f : INT32_MIN;
}
__host__ __device__ inline int32_t go_i32(double d)
{
    return (d > -2147483649.0 && d < 2147483648.0) ? (int32_t)d : INT32_MIN;
}

}  // namespace nl
