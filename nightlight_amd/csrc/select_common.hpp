// select_common.hpp -- what the operators that select order statistics share (background.hip, deband.hip): the
// order-preserving float <-> uint32 keys, the workgroup radix select over them, and the host's literal QSelectFloat32 /
// QSelectMedianFloat32 with Go's bounds checks.  For NaN-free samples an order statistic is a function of the multiset
// only, so the reference's in-place reordering cannot change it (up to the sign of a zero tied at the selected rank).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "frame_common.hpp"

namespace nl {

constexpr int kSelectThreads = 256;    // four waves per selection

__device__ inline uint32_t f2key(float f)
{
    const uint32_t u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float key2f(uint32_t k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

// block-wide reductions of kSelectThreads lanes through red[4] (LDS); every lane gets the result
__device__ inline unsigned block_sum(unsigned v, unsigned *red)
{
    v = wave_sum(v);
    __syncthreads();                   // (red may still be read from the reduction before)
    wave_values(v, red);
    return sum_in_order<kSelectThreads / 64>(red);
}
__device__ inline unsigned block_max(unsigned v, unsigned *red)
{
    v = wave_max(v);
    __syncthreads();
    wave_values(v, red);
    return max(max(red[0], red[1]), max(red[2], red[3]));
}

struct SelectShared {
    unsigned hist[256];
    unsigned red[4];
    unsigned bucket, below, count, nan;
};

// Key of the k-th smallest (1-based, 1 <= k <= members) member: get(i, &key) says whether sample i is a member.
template <class Get>
__device__ uint32_t block_select(int n, unsigned k, Get get, SelectShared &sh)
{
    uint32_t prefix = 0, mask = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        sh.hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += kSelectThreads) {
            uint32_t key;
            if (get(i, &key) && (key & mask) == prefix) atomicAdd(&sh.hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        // inclusive scan of the 256 bins, one per lane
        const unsigned c = sh.hist[threadIdx.x];
        unsigned incl = c;
        const int lane = threadIdx.x & 63;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(incl, d, 64);
            if (lane >= d) incl += t;
        }
        if (lane == 63) sh.red[threadIdx.x >> 6] = incl;
        __syncthreads();
        for (int wv = 0; wv < (int)(threadIdx.x >> 6); wv++) incl += sh.red[wv];
        if (incl >= k && incl - c < k) { sh.bucket = threadIdx.x; sh.below = incl - c; }
        __syncthreads();
        k -= sh.below;
        prefix |= sh.bucket << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// QSelectFloat32 (qsort.go:94-126), literally, with Go's bounds checks: false where the reference panics
inline bool qselect_lit(float *a, int n, int k, float *out)
{
    int left = 0, right = n - 1;
    while (left < right) {
        const int mid = (left + right) >> 1;
        const float pivot = a[mid];
        int l = left - 1, r = right + 1;
        for (;;) {
            do { if (++l >= n) return false; } while (!(a[l] >= pivot));
            do { if (--r < 0) return false; } while (!(a[r] <= pivot));
            if (l >= r) break;
            std::swap(a[l], a[r]);
        }
        const int index = r;
        const int offset = index - left + 1;
        if (k <= offset) right = index;
        else { left = index + 1; k -= offset; }
    }
    if (left < 0 || left >= n) return false;
    *out = a[left];
    return true;
}

// QSelectMedianFloat32 (qsort.go:68-82), literally
inline bool qselect_median_lit(float *a, int n, float *out)
{
    const int k = (n >> 1) + 1;
    float upper;
    if (!qselect_lit(a, n, k, &upper)) return false;
    if (n & 1) { *out = upper; return true; }
    float lower = a[0];
    for (int i = 1; i < k - 1; i++)
        if (a[i] > lower) lower = a[i];
    *out = 0.5f * (lower + upper);
    return true;
}

}  // namespace nl
