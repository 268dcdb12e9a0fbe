// quad_common.hpp -- what the per-pixel kernels of tone.hip and colour.hip share: a frame walked in quads (16-byte
// loads and stores where the pointer allows, the same quads element by element where it does not), the in-place
// transform that also reduces what it writes in min_sum_max_kernel's partition, the fp64 power narrowed once, and
// OpSave's count of one pixel.  Device code and its launch geometry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "frame_common.hpp"

namespace nl {

// float32(math.Pow(float64(x), gg))
__device__ __forceinline__ float pow_f32(float x, double gg)
{
    return (float)pow((double)x, gg);
}

// pixels 4q ... 4q + 3
template <bool VEC>
__device__ __forceinline__ float4 load_quad(const float *data, int64_t q)
{
    if constexpr (VEC) return reinterpret_cast<const float4 *>(data)[q];
    const float *s = data + (q << 2);
    return make_float4(s[0], s[1], s[2], s[3]);
}

template <bool VEC>
__device__ __forceinline__ void store_quad(float *data, int64_t q, float4 v)
{
    if constexpr (VEC) {
        reinterpret_cast<float4 *>(data)[q] = v;
    } else {
        float *s = data + (q << 2);
        s[0] = v.x;
        s[1] = v.y;
        s[2] = v.z;
        s[3] = v.w;
    }
}

// data[i] = f(data[i]) over n floats, by a workgroup of 256 lanes of a 1-D grid in x.  STATS: min / max in fp32 by
// explicit compares, sum in fp64, over the values written, in the partition and the order of min_sum_max_kernel
// (frame_stats.hip) -- a grid stride over quads, the tail by lane 0 of workgroup 0 -- so that the partials are the ones
// that kernel would leave on the transformed frame; *seed = f(data[0]) as it was before this launch.
template <bool STATS, bool VEC, class F>
__device__ __forceinline__ void quad_transform(float *data, int64_t n, F f, const float *seed, double *partial)
{
    float mn = 0.0f, mx = 0.0f;
    double sum = 0.0;
    if constexpr (STATS) mn = mx = *seed;
    const int64_t quads = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = load_quad<VEC>(data, q);
        float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            e[j] = f(e[j]);
            if constexpr (STATS) {
                if (e[j] < mn) mn = e[j];
                if (e[j] > mx) mx = e[j];
                sum += (double)e[j];
            }
        }
        store_quad<VEC>(data, q, make_float4(e[0], e[1], e[2], e[3]));
    }
    if constexpr (STATS) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            for (int64_t i = quads << 2; i < n; i++) {
                const float e = f(data[i]);
                data[i] = e;
                if (e < mn) mn = e;
                if (e > mx) mx = e;
                sum += (double)e;
            }
        }
        block_min_sum_max(mn, sum, mx, partial);
    } else if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (quads << 2) + threadIdx.x;
        data[i] = f(data[i]);
    }
}

// tiff16.go:58-85, :116-132 / writejpg.go:56-83, :114-128 up to the conversion: the count of one pixel of one channel,
// 0 ... 65535 or 0 ... 255
template <int BITS, bool GAMMA>
__device__ __forceinline__ unsigned gray_count(float d, float min, float scale, double gamma_inv)
{
    float gray = (d - min) * scale;
    if (gray != gray || gray < 0.0f) gray = 0.0f;
    if (gray > 1.0f) gray = 1.0f;
    if constexpr (GAMMA) gray = pow_f32(gray, gamma_inv);
    return (unsigned)(gray * (BITS == 16 ? 65535.0f : 255.0f));         // 0 <= gray <= 1: truncation, in range
}

// workgroups of 256 lanes for a grid stride over the quads of n pixels
inline int quad_blocks(int64_t n)
{
    const int64_t want = ((n >> 2) + 255) / 256;
    return (int)(want < 1 ? 1 : (want > 16384 ? 16384 : want));
}

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace nl
