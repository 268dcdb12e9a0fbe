// drizzle.hip -- drizzle integration of a resident, unresampled frame onto an output grid of another scale, for
// nl_stack_frame_drizzle_from, and the two elementwise steps around it: nl_stack_drizzle_finalize's quotient and
// nl_stack_frame_reject_against's blot-and-compare.  AN EXTENSION: the reference has no drizzle;
// include/nlstack_drizzle.h carries the definition these kernels compute bit for bit.
//
// The gather form: one output pixel per work item, which walks the (2R + 1)^2 source pixels around its own rounded
// source position in a fixed order and adds the overlap of each one's drop with itself.  No atomics, so the planes are
// deterministic, and a frame is laid down in one pass over the output.
//
// The structure is project.hip's (the walk itself is written once, in drizzle_walk.hpp, for this unit, drizzle_cfa.hip
// and drizzle_square.hip; this unit gives it the weight of a NL_DZ_TURBO / NL_DZ_POINT candidate).  A workgroup owns a kProjTileW x kProjTileH tile of the output; wave w makes rows w,
// w + 4, ... of it, lane l the columns l, l + 64, l + 128, l + 192 of a row, so every load and store of the two planes
// covers 256 contiguous bytes per wave.  From the four corners of its tile (drizzle.hpp) the workgroup computes the
// candidate box of the tile; it stages the box in LDS (each source byte fetched once, 16 bytes per lane where the
// source's width allows) when the box is within kDzLdsFloats, else every candidate comes from global memory.  On a
// finer output grid the box is small: 256 x 16 output pixels at scale 2 are 128 x 8 source pixels plus the window.
//
// Most candidates of a window fail the overlap test.  Nothing branches on that: a candidate that is outside the
// source, or whose drop misses the pixel, reads element 0 (always there) and carries a NaN as its weight, which the
// sums drop by a select as they drop a pixel without data (weight is finite, so no real candidate has one); the
// (2R + 1)^2 loads of a pixel are independent and in flight together, and no mask outlives its candidate.  A pixel
// whose whole window misses the source skips the loop.
//
// Bit-exact: coordinates, overlaps and sums in the header's operand order, no FMA (-ffp-contract=off).
#include <math.h>

#include "drizzle.hpp"
#include "drizzle_walk.hpp"
#include "frame_common.hpp"
#include "launch_common.hpp"

namespace nl {

namespace {

// flags: drizzle_walk.hpp's drizzle_tile
template <int R, bool POINT>
__global__ __launch_bounds__(256) void drizzle_tile_kernel(const float *__restrict__ src, int src_w, int src_h,
                                                           float *__restrict__ sum, float *__restrict__ wgt, int dst_w,
                                                           int row0, int rows, DzGeom q, float weight, unsigned flags)
{
    __shared__ float lds[kDzLdsFloats];
    drizzle_tile<R>(lds, src, src_w, src_h, sum, wgt, dst_w, row0, rows, q.g, DzDrop<POINT>{q, weight}, flags);
}

__global__ __launch_bounds__(256) void drizzle_finalize_kernel(const float *sum, const float *wgt, float *out, int64_t n,
                                                                float min_weight, float empty)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float s = sum[i], w = wgt[i];
        out[i] = w > min_weight ? s / w : empty;                             // (a NaN weight: empty)
    }
}

__global__ __launch_bounds__(256) void reject_against_kernel(float *frame, const float *model, int64_t n,
                                                              float low, float high, unsigned long long *counts)
{
    unsigned n_low = 0, n_high = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float d = frame[i] - model[i];
        const bool is_low = d < -low, is_high = !is_low && d > high;         // (a NaN on either side: neither)
        if (is_low || is_high) frame[i] = __builtin_nanf("");
        n_low += is_low ? 1u : 0u;
        n_high += is_high ? 1u : 0u;
    }
    __shared__ unsigned s_low[4], s_high[4];
    n_low = wave_sum(n_low);
    n_high = wave_sum(n_high);
    if ((threadIdx.x & 63) == 0) { s_low[threadIdx.x >> 6] = n_low; s_high[threadIdx.x >> 6] = n_high; }
    __syncthreads();
    if (threadIdx.x == 0) {
        counts[2 * (size_t)blockIdx.x + 0] = (unsigned long long)sum_in_order<4>(s_low);
        counts[2 * (size_t)blockIdx.x + 1] = (unsigned long long)sum_in_order<4>(s_high);
    }
}

unsigned stream_grid(int64_t n)
{
    const int64_t g = (n + 255) / 256;
    return (unsigned)(g > 256 * 32 ? 256 * 32 : (g < 1 ? 1 : g));
}

}  // namespace

hipError_t launch_drizzle(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0, int rows,
                          const DzGeom &geom, float weight, bool first, bool point, unsigned switches, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + kProjTileW - 1) / kProjTileW), (unsigned)((rows + kProjTileH - 1) / kProjTileH));
    const unsigned flags = dz_tile_flags(src, src_w, switches) | (first ? 4u : 0u);
    Launcher L(stream);
    with_class<1, 2, 3>(geom.radius, [&](auto R) {
        with_bool(point, [&](auto P) {
            L(drizzle_tile_kernel<decltype(R)::value, decltype(P)::value>, grid, 256, 0, src, src_w, src_h, sum, wgt, dst_w,
              row0, rows, geom, weight, flags);
        });
    });
    return L.err;
}

void drizzle_tile_paths(const float *src, int src_w, int src_h, int dst_w, int row0, int rows, const DzGeom &geom,
                        unsigned switches, int64_t *staged, int64_t *direct)
{
    const unsigned flags = dz_tile_flags(src, src_w, switches);
    int64_t n_staged = 0, n_direct = 0;
    for (int r0 = 0; r0 < rows; r0 += kProjTileH)
        for (int c0 = 0; c0 < dst_w; c0 += kProjTileW) {
            const int c1 = (c0 + kProjTileW < dst_w ? c0 + kProjTileW : dst_w) - 1;
            const int r_end = r0 + kProjTileH < rows ? r0 + kProjTileH : rows;
            ProjBox b;
            if ((flags & 2u) && dz_tile_box(geom.g, geom.radius, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, flags & 1u, b))
                n_staged++;
            else
                n_direct++;
        }
    *staged = n_staged;
    *direct = n_direct;
}

hipError_t launch_drizzle_finalize(const float *sum, const float *wgt, float *out, int64_t n, float min_weight, float empty,
                                   hipStream_t stream)
{
    Launcher L(stream);
    L(drizzle_finalize_kernel, stream_grid(n), 256, 0, sum, wgt, out, n, min_weight, empty);
    return L.err;
}

hipError_t launch_reject_against(float *frame, const float *model, int64_t n, float low, float high,
                                 unsigned long long *counts, int blocks, hipStream_t stream)
{
    Launcher L(stream);
    L(reject_against_kernel, (unsigned)blocks, 256, 0, frame, model, n, low, high, counts);
    return L.err;
}

}  // namespace nl
