// drizzle_walk.hpp -- the walks of the drizzle's tile kernels, written once: what a workgroup does for its tile of the
// output (the candidate box, its staging in LDS, the rows of the tile) in the mono form of drizzle.hip and in the strided
// CFA form of drizzle_cfa.hip, with the weight of a candidate left to a template parameter.  drizzle.hip and
// drizzle_cfa.hip instantiate them with DzDrop (NL_DZ_TURBO / NL_DZ_POINT, drizzle.hpp's dz_candidate_weight),
// drizzle_square.hip with its rotated drop.  The comments on the structure are in those units.
//
// Cand: cand(fi, fj, px, py, ok) is the weight wa that source pixel (fi, fj) lays onto output pixel (px, py), in the
// header's operand order.  ok comes in as "a pixel the walk takes" (inside the source; of the channel) and leaves as "a
// candidate": a NaN weight marks the ones that are not.
#pragma once
#include <math.h>

#include "drizzle.hpp"
#include "frame_common.hpp"

namespace nl {

// NL_DZ_TURBO / NL_DZ_POINT of include/nlstack_drizzle.h
template <bool POINT>
struct DzDrop {
    const DzGeom &q;
    float weight;
    __device__ __forceinline__ float operator()(float fi, float fj, float px, float py, bool &ok) const
    {
        return dz_candidate_weight<POINT>(q, fi, fj, px, py, weight, ok);
    }
};

// rows of the tile for this wave, four pixels per lane and row.  mem = the box in LDS (origin org_x, org_y, pitch
// b.pitch) or the source itself (origin 0, 0, pitch src_w).
template <int R, class Cand, class Index>
__device__ __forceinline__ void drizzle_rows(const float *__restrict__ mem, int org_x, int org_y, Index pitch, int src_w,
                                             int src_h, float *__restrict__ sum, float *__restrict__ wgt, int dst_w,
                                             int row0, int c0, int r_first, int r_end, const ProjInv &g, const Cand &cand,
                                             bool first)
{
    const int lane = threadIdx.x & 63;
    // xc in [-R, src_w - 1 + R] or the window misses the source (the bound may round up: every candidate is tested)
    const float x_last = fminf((float)src_w + (float)R, 2147483520.0f), y_last = fminf((float)src_h + (float)R, 2147483520.0f);
    for (int r = r_first + (int)(threadIdx.x >> 6); r < r_end; r += 4) {
        const float py = (float)(row0 + r);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = c0 + lane + 64 * k;
            if (col >= dst_w) continue;
            const float px = (float)col;
            const float X = proj_x(g, px, py), Y = proj_y(g, px, py);
            const float xc = floorf(X + 0.5f), yc = floorf(Y + 0.5f);
            const int64_t at = (int64_t)r * dst_w + col;
            float s = 0.0f, t = 0.0f;
            if (!first) { s = sum[at]; t = wgt[at]; }
            // (a NaN fails every comparison: no candidates)
            if (xc >= -(float)R && xc <= x_last && yc >= -(float)R && yc <= y_last) {
                const int xi = (int)xc, yi = (int)yc;
                float v[2 * R + 1][2 * R + 1], wa[2 * R + 1][2 * R + 1];
#pragma unroll
                for (int dj = 0; dj <= 2 * R; dj++) {
                    const int j = yi + dj - R;
                    const float fj = (float)j;
#pragma unroll
                    for (int di = 0; di <= 2 * R; di++) {
                        const int i = xi + di - R;
                        const float fi = (float)i;
                        bool ok = (unsigned)i < (unsigned)src_w && (unsigned)j < (unsigned)src_h;
                        wa[dj][di] = cand(fi, fj, px, py, ok);
                        const Index p = ok ? (Index)(j - org_y) * pitch + (Index)(i - org_x) : (Index)0;
                        v[dj][di] = mem[p];
                    }
                }
#pragma unroll
                for (int dj = 0; dj <= 2 * R; dj++) {
#pragma unroll
                    for (int di = 0; di <= 2 * R; di++) {
                        const float x = v[dj][di];
                        const bool ok = x == x && wa[dj][di] == wa[dj][di]; // NaN = no data; a NaN weight = no candidate
                        const float sn = s + x * wa[dj][di], tn = t + wa[dj][di];
                        s = ok ? sn : s;
                        t = ok ? tn : t;
                    }
                }
            }
            sum[at] = s;
            wgt[at] = t;
        }
    }
}

// drizzle_rows over the channel's positions of each window (drizzle_cfa.hip: the strided window)
template <int R, class Cand, bool GREEN, class Index>
__device__ __forceinline__ void drizzle_cfa_rows(const float *__restrict__ mem, int org_x, int org_y, Index pitch, int src_w,
                                                 int src_h, float *__restrict__ sum, float *__restrict__ wgt, int dst_w,
                                                 int row0, int c0, int r_first, int r_end, const ProjInv &g, const Cand &cand,
                                                 bool first, const DzChannel &ch)
{
    constexpr int NR = GREEN ? 2 * R + 1 : R + 1, NC = R + 1;
    const int lane = threadIdx.x & 63;
    const float x_last = fminf((float)src_w + (float)R, 2147483520.0f), y_last = fminf((float)src_h + (float)R, 2147483520.0f);
    for (int r = r_first + (int)(threadIdx.x >> 6); r < r_end; r += 4) {
        const float py = (float)(row0 + r);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int col = c0 + lane + 64 * k;
            if (col >= dst_w) continue;
            const float px = (float)col;
            const float X = proj_x(g, px, py), Y = proj_y(g, px, py);
            const float xc = floorf(X + 0.5f), yc = floorf(Y + 0.5f);
            const int64_t at = (int64_t)r * dst_w + col;
            float s = 0.0f, t = 0.0f;
            if (!first) { s = sum[at]; t = wgt[at]; }
            if (xc >= -(float)R && xc <= x_last && yc >= -(float)R && yc <= y_last) {
                const int xi = (int)xc, yi = (int)yc;
                const int wx = xi - R, wy = yi - R, x_end = xi + R, y_end = yi + R;      // (x_end + 1 stays an int)
                // the first row / column of the channel's parity at or behind the window's start
                const int j_first = GREEN ? wy : wy + ((wy ^ ch.par_y) & 1);
                const int i_sparse = wx + ((wx ^ ch.par_x) & 1);
                float v[NR][NC], wa[NR][NC];
#pragma unroll
                for (int dj = 0; dj < NR; dj++) {
                    const int j = GREEN ? j_first + dj : j_first + 2 * dj;
                    const float fj = (float)j;
                    const int i_first = GREEN ? wx + ((wx ^ j ^ ch.par_x) & 1) : i_sparse;
                    const bool row_ok = (GREEN || j <= y_end) && j >= ch.yo && j < src_h;
#pragma unroll
                    for (int di = 0; di < NC; di++) {
                        const int i = i_first + 2 * di;
                        const float fi = (float)i;
                        bool ok = row_ok && i <= x_end && i >= ch.xo && i < src_w;
                        wa[dj][di] = cand(fi, fj, px, py, ok);
                        const Index p = ok ? (Index)(j - org_y) * pitch + (Index)(i - org_x) : (Index)0;
                        v[dj][di] = mem[p];
                    }
                }
#pragma unroll
                for (int dj = 0; dj < NR; dj++) {
#pragma unroll
                    for (int di = 0; di < NC; di++) {
                        const float x = v[dj][di];
                        const bool ok = x == x && wa[dj][di] == wa[dj][di]; // NaN = no data; a NaN weight = no candidate
                        const float sn = s + x * wa[dj][di], tn = t + wa[dj][di];
                        s = ok ? sn : s;
                        t = ok ? tn : t;
                    }
                }
            }
            sum[at] = s;
            wgt[at] = t;
        }
    }
}

// A workgroup's tile of the mono walk: the candidate box, staged in lds (kDzLdsFloats floats) where it fits, and the
// rows.  flags: bit 0 = the source allows 16-byte loads, bit 1 = tiles may stage their box, bit 2 = first
template <int R, class Cand>
__device__ __forceinline__ void drizzle_tile(float *lds, const float *__restrict__ src, int src_w, int src_h,
                                             float *__restrict__ sum, float *__restrict__ wgt, int dst_w, int row0, int rows,
                                             const ProjInv &g, const Cand &cand, unsigned flags)
{
    const int c0 = blockIdx.x * kProjTileW, r0 = blockIdx.y * kProjTileH;
    const int c1 = min(c0 + kProjTileW, dst_w) - 1, r_end = min(r0 + kProjTileH, rows);
    const bool vec = flags & 1u, first = flags & 4u;
    ProjBox b = {0, 0, 0, 0, 0};
    const bool staged = (flags & 2u) && dz_tile_box(g, R, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, vec, b);
    if (staged) {                                                            // (uniform over the workgroup)
        if (vec) stage_box<true>(src, src_w, b, lds);
        else stage_box<false>(src, src_w, b, lds);
        __syncthreads();
        drizzle_rows<R, Cand, int>(lds, b.x0, b.y0, b.pitch, src_w, src_h, sum, wgt, dst_w, row0, c0, r0, r_end, g, cand, first);
    } else {
        drizzle_rows<R, Cand, int64_t>(src, 0, 0, src_w, src_w, src_h, sum, wgt, dst_w, row0, c0, r0, r_end, g, cand, first);
    }
}

// the same of the CFA walk
template <int R, class Cand, bool GREEN>
__device__ __forceinline__ void drizzle_cfa_tile(float *lds, const float *__restrict__ src, int src_w, int src_h,
                                                 float *__restrict__ sum, float *__restrict__ wgt, int dst_w, int row0,
                                                 int rows, const ProjInv &g, const Cand &cand, unsigned flags,
                                                 const DzChannel &ch)
{
    const int c0 = blockIdx.x * kProjTileW, r0 = blockIdx.y * kProjTileH;
    const int c1 = min(c0 + kProjTileW, dst_w) - 1, r_end = min(r0 + kProjTileH, rows);
    const bool vec = flags & 1u, first = flags & 4u;
    ProjBox b = {0, 0, 0, 0, 0};
    const bool staged = (flags & 2u) && dz_tile_box(g, R, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, vec, b);
    if (staged) {                                                            // (uniform over the workgroup)
        if (vec) stage_box<true>(src, src_w, b, lds);
        else stage_box<false>(src, src_w, b, lds);
        __syncthreads();
        drizzle_cfa_rows<R, Cand, GREEN, int>(lds, b.x0, b.y0, b.pitch, src_w, src_h, sum, wgt, dst_w, row0, c0, r0, r_end, g,
                                              cand, first, ch);
    } else {
        drizzle_cfa_rows<R, Cand, GREEN, int64_t>(src, 0, 0, src_w, src_w, src_h, sum, wgt, dst_w, row0, c0, r0, r_end, g,
                                                  cand, first, ch);
    }
}

}  // namespace nl
