// drizzle_cfa.hip -- CFA drizzle: the pixels of one channel of a raw Bayer mosaic laid onto that colour's flux and weight
// plane with no debayer in front, for nl_stack_frame_drizzle_cfa_from, and nl_stack_frame_reject_against_cfa's stream.
// AN EXTENSION: include/nlstack_cfadrizzle.h carries the definition -- nlstack_drizzle.h's, with one addition: a
// candidate that is not a pixel of the channel is skipped -- which these kernels compute bit for bit.
//
// A sibling of drizzle.hip's tile kernel in a unit of its own, so that the six mono instantiations keep their code
// (DESIGN.md section 6u's table).  The walk described below is drizzle_walk.hpp's drizzle_cfa_rows.  The tile shape, the candidate box, its staging in LDS (the whole box, all colours:
// drizzle_tile_paths() answers for this kernel too) and a candidate's arithmetic (dz_candidate_weight) are drizzle.hpp's.
//
// The strided window.  A work item does not test the (2R + 1)^2 pixels of its window for their colour: it walks the
// channel's positions only.  R and B: the first row of the window with the channel's row parity, then every second
// row, at most R + 1 of them, and the same per column -- (R + 1)^2 candidates (4 / 9 / 16 instead of 9 / 25 / 49).
// G: all 2R + 1 rows, in row j from the first column of the parity the row asks for, then every second column --
// (2R + 1)(R + 1) candidates (6 / 15 / 28).  Rows outer, columns inner, both rising: the order of the surviving
// candidates is the definition's, so no bit moves.  A stride step that runs past the window, falls outside the source
// or lies in front of (xo, yo) is masked as drizzle.hip masks: element 0 and a NaN weight; no predicate outlives its
// candidate.  Window starts are negative for frames partly outside the grid: parities are taken with & 1.
#include <math.h>

#include "drizzle.hpp"
#include "drizzle_walk.hpp"
#include "frame_common.hpp"
#include "launch_common.hpp"

namespace nl {

namespace {

// flags: drizzle_walk.hpp's drizzle_tile
template <int R, bool POINT, bool GREEN>
__global__ __launch_bounds__(256) void drizzle_cfa_tile_kernel(const float *__restrict__ src, int src_w, int src_h,
                                                               float *__restrict__ sum, float *__restrict__ wgt, int dst_w,
                                                               int row0, int rows, DzGeom q, float weight, unsigned flags,
                                                               DzChannel ch)
{
    __shared__ float lds[kDzLdsFloats];
    drizzle_cfa_tile<R, DzDrop<POINT>, GREEN>(lds, src, src_w, src_h, sum, wgt, dst_w, row0, rows, q.g, DzDrop<POINT>{q, weight},
                                              flags, ch);
}

// nl_stack_frame_reject_against's test on one pixel, and its counting: the wave sums, then the four wave values in
// order into counts[2 * blockIdx.x] / [+ 1] (reject_against_kernel of drizzle.hip, which stays as it is)
__device__ __forceinline__ void reject_pixel(float *v, float m, float low, float high, unsigned &n_low, unsigned &n_high)
{
    const float d = *v - m;
    const bool is_low = d < -low, is_high = !is_low && d > high;             // (a NaN on either side: neither)
    if (is_low || is_high) *v = __builtin_nanf("");
    n_low += is_low ? 1u : 0u;
    n_high += is_high ? 1u : 0u;
}

__device__ __forceinline__ void reject_counts(unsigned n_low, unsigned n_high, unsigned long long *counts)
{
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

// workgroup b takes the rows b, b + gridDim.x, ... of the tile; a work item the columns threadIdx.x, + 256, ...
__global__ __launch_bounds__(256) void reject_against_cfa_kernel(float *frame, const float *model, int width, int row0,
                                                                  int rows, DzChannel ch, float low, float high,
                                                                  unsigned long long *counts)
{
    unsigned n_low = 0, n_high = 0;
    for (int r = blockIdx.x; r < rows; r += gridDim.x) {
        const int64_t at = (int64_t)r * width;
        for (int i = threadIdx.x; i < width; i += 256)
            if (dz_channel_has(ch, i, row0 + r)) reject_pixel(frame + at + i, model[at + i], low, high, n_low, n_high);
    }
    reject_counts(n_low, n_high, counts);
}

}  // namespace

hipError_t launch_drizzle_cfa(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0, int rows,
                              const DzGeom &geom, float weight, bool first, bool point, const DzChannel &ch,
                              unsigned switches, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + kProjTileW - 1) / kProjTileW), (unsigned)((rows + kProjTileH - 1) / kProjTileH));
    const unsigned flags = dz_tile_flags(src, src_w, switches) | (first ? 4u : 0u);
    Launcher L(stream);
    with_class<1, 2, 3>(geom.radius, [&](auto R) {
        with_bool(point, [&](auto P) {
            with_bool(ch.green != 0, [&](auto G) {
                L(drizzle_cfa_tile_kernel<decltype(R)::value, decltype(P)::value, decltype(G)::value>, grid, 256, 0, src, src_w,
                  src_h, sum, wgt, dst_w, row0, rows, geom, weight, flags, ch);
            });
        });
    });
    return L.err;
}

hipError_t launch_reject_against_cfa(float *frame, const float *model, int width, int row0, int rows, const DzChannel &ch,
                                     float low, float high, unsigned long long *counts, int blocks, hipStream_t stream)
{
    Launcher L(stream);
    L(reject_against_cfa_kernel, (unsigned)blocks, 256, 0, frame, model, width, row0, rows, ch, low, high, counts);
    return L.err;
}

}  // namespace nl
