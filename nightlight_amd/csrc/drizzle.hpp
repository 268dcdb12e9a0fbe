// drizzle.hpp -- what the kernels of drizzle.hip, drizzle_cfa.hip and drizzle_square.hip, their launchers and the entries (nlstack_drizzle.hip) share: the geometry of
// include/nlstack_drizzle.h as the kernel takes it, the candidate box of an output tile -- the one piece of arithmetic
// host and device both run (the same fp32 operations, no contraction on either side, so drizzle_tile_paths() counts
// exactly the tiles the kernel stages) -- and the launchers.  ProjInv, ProjBox, stage_box and the tile shape are
// project.hpp's.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "bayer.hpp"
#include "project.hpp"

namespace nl {

constexpr int kDzLdsFloats = 8192;        // 32 KiB: five workgroups (20 waves) share a CU's 160 KiB
constexpr int kDzMaxRadius = 3;           // NL_DZ_MAX_RADIUS

// nl_drizzle_geometry's results: f = source -> output pixel, g = output -> source pixel, hw = half the drop's side in
// output pixels, radius = R of the candidate window
struct DzGeom {
    ProjInv f, g;
    float hw;
    int radius;
};

// what nl_drizzle_square_geometry adds (include/nlstack_sqdrizzle.h): the corners of a drop relative to its centre, in
// output pixels and in the order that makes the edge sum positive, and the half-sides of the drop's bounding box.  It
// travels beside DzGeom (whose radius is then the square R), so that the kernels of drizzle.hip and drizzle_cfa.hip keep
// their arguments.
struct DzSquare {
    float cx[4], cy[4];
    float bx, by;
};

// floor(v + 0.5f) as an int where it matters: anything below -8 is -8 (its window of radius <= 3 ends in front of
// column 0 either way), anything above 2^31 - 128 is that (behind every source, and +- 3 stays an int); v is no NaN
__host__ __device__ inline int dz_round_clamped(float v)
{
    const float f = floorf(v + 0.5f);
    return (int)(f < -8.0f ? -8.0f : (f > 2147483520.0f ? 2147483520.0f : f));
}

// The candidate box of the output tile of columns [c0, c1] and image rows [r0, r1] (inclusive): every source pixel in
// the window of radius R around the rounded source position of a pixel of the tile.  False when the tile takes its
// candidates from global memory instead: a coordinate that is NaN at a corner, a box beyond the LDS budget, or no
// candidate in the source at all (then nothing is read either way).
//
// The four corners are enough, with no margin, by project.hpp's argument: X = fl(fl(fl(a*px) + fl(b*py)) + c) is
// monotone in px for a fixed py and in py for a fixed px, rounding included, and so are fl(X + 0.5f) and its floor;
// the smallest and the largest xc over the rectangle are taken at corners.  Same for yc.
//
// Unlike proj_tile_box a candidate needs no 2x2 footprint: the box reaches the source's last column and row, and one
// pixel of it is enough.
__host__ __device__ inline bool dz_tile_box(const ProjInv &g, int radius, int src_w, int src_h, int c0, int c1, int r0,
                                            int r1, bool vec, ProjBox &b)
{
    const float px0 = (float)c0, px1 = (float)c1, py0 = (float)r0, py1 = (float)r1;
    const float x00 = proj_x(g, px0, py0), x10 = proj_x(g, px1, py0), x01 = proj_x(g, px0, py1), x11 = proj_x(g, px1, py1);
    const float y00 = proj_y(g, px0, py0), y10 = proj_y(g, px1, py0), y01 = proj_y(g, px0, py1), y11 = proj_y(g, px1, py1);
    if (x00 != x00 || x10 != x10 || x01 != x01 || x11 != x11 || y00 != y00 || y10 != y10 || y01 != y01 || y11 != y11)
        return false;
    const float xmin = fminf(fminf(x00, x10), fminf(x01, x11)), xmax = fmaxf(fmaxf(x00, x10), fmaxf(x01, x11));
    const float ymin = fminf(fminf(y00, y10), fminf(y01, y11)), ymax = fmaxf(fmaxf(y00, y10), fmaxf(y01, y11));
    int x0 = dz_round_clamped(xmin) - radius, x1 = dz_round_clamped(xmax) + radius;
    int y0 = dz_round_clamped(ymin) - radius, y1 = dz_round_clamped(ymax) + radius;
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > src_w - 1) x1 = src_w - 1;
    if (y1 > src_h - 1) y1 = src_h - 1;
    if (x1 < x0 || y1 < y0) return false;                  // no candidate in the source
    if (vec) {                                             // whole 16-byte groups of a row (src_w is a multiple of 4)
        x0 &= ~3;
        x1 |= 3;
    }
    b.x0 = x0;
    b.y0 = y0;
    b.w = x1 - x0 + 1;
    b.h = y1 - y0 + 1;
    b.pitch = b.w | 1;                                     // odd, as proj_tile_box: a quarter turn spreads over the banks
    return (int64_t)b.pitch * b.h <= kDzLdsFloats;
}

// One candidate of the definition, what drizzle.hip's and drizzle_cfa.hip's walks share: the weight wa that source
// pixel (fi, fj) lays onto output pixel (px, py), in the header's operand order.  ok comes in as "a pixel the walk
// takes" (inside the source; of the channel) and leaves as "a candidate": a NaN weight marks the ones that are not.
template <bool POINT>
__device__ __forceinline__ float dz_candidate_weight(const DzGeom &q, float fi, float fj, float px, float py, float weight,
                                                     bool &ok)
{
    const float u = proj_x(q.f, fi, fj), vv = proj_y(q.f, fi, fj);
    if constexpr (POINT) {
        ok = ok && floorf(u + 0.5f) == px && floorf(vv + 0.5f) == py;
        return ok ? weight : __builtin_nanf("");
    } else {
        float lo = u - q.hw, e = px - 0.5f;
        if (e > lo) lo = e;
        float hi = u + q.hw;
        e = px + 0.5f;
        if (e < hi) hi = e;
        const float ox = hi - lo;
        lo = vv - q.hw;
        e = py - 0.5f;
        if (e > lo) lo = e;
        hi = vv + q.hw;
        e = py + 0.5f;
        if (e < hi) hi = e;
        const float oy = hi - lo;
        ok = ok && ox > 0.0f && oy > 0.0f;
        const float ar = ox * oy;
        return ok ? weight * ar : __builtin_nanf("");
    }
}

// bits 0 / 1 of the tile kernels' flags (project.hip's rule; the geometry's coefficients are finite): the source allows
// 16-byte loads, tiles may stage their box
inline unsigned dz_tile_flags(const float *src, int src_w, unsigned switches)
{
    const bool vec = (src_w & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    return (vec ? 1u : 0u) | (!(switches & kProjDirectOnly) ? 2u : 0u);
}

// The pixels of one channel of a raw mosaic (include/nlstack_cfadrizzle.h): (i, j) with i >= xo, j >= yo and, for R and
// B, i of parity par_x and j of parity par_y; for G, i + j of parity par_x.  Parities are taken with & 1, which holds
// for the negative window starts of a frame partly outside the grid as well (two's complement); % would not.
struct DzChannel {
    int xo, yo;            // getOffsets (debayer.go:26-37)
    int green;             // 1 for G
    int par_x, par_y;
};

// channel: bayer.hpp's BayerChannel
inline DzChannel dz_channel(int channel, int xo, int yo)
{
    if (channel == kBayerG) return {xo, yo, 1, (xo + yo + 1) & 1, 0};
    const int b = channel == kBayerB ? 1 : 0;
    return {xo, yo, 0, (xo + b) & 1, (yo + b) & 1};
}

__host__ __device__ inline bool dz_channel_has(const DzChannel &c, int i, int j)
{
    const bool par = c.green ? ((i + j) & 1) == c.par_x : ((i & 1) == c.par_x && (j & 1) == c.par_y);
    return i >= c.xo && j >= c.yo && par;
}

// ---- drizzle_cfa.hip ----
// nl_stack_frame_drizzle_cfa_from's kernel: launch_drizzle over the pixels of channel ch of the mosaic src only, the
// strided walk of the window
hipError_t launch_drizzle_cfa(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0, int rows,
                              const DzGeom &geom, float weight, bool first, bool point, const DzChannel &ch,
                              unsigned switches, hipStream_t stream);
// nl_stack_frame_reject_against_cfa's kernel: launch_reject_against on the channel's pixels of the rows [row0, row0 +
// rows) of a width wide mosaic
hipError_t launch_reject_against_cfa(float *frame, const float *model, int width, int row0, int rows, const DzChannel &ch,
                                     float low, float high, unsigned long long *counts, int blocks, hipStream_t stream);

// ---- drizzle_square.hip ----
// nl_stack_frame_drizzle_square_from's kernel: launch_drizzle with the exact overlap of the rotated drop as a
// candidate's area.  switches: kProjDirectOnly, and kDzSquareEveryCandidate (developer switch 262144 of
// nl_stack_set_dev_flags) = the four edges of every candidate are evaluated, none skipped wave by wave; the same bits
constexpr unsigned kDzSquareEveryCandidate = 4u;
hipError_t launch_drizzle_square(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0,
                                 int rows, const DzGeom &geom, const DzSquare &sq, float weight, bool first,
                                 unsigned switches, hipStream_t stream);
// nl_stack_frame_drizzle_square_cfa_from's: launch_drizzle_cfa likewise
hipError_t launch_drizzle_square_cfa(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0,
                                     int rows, const DzGeom &geom, const DzSquare &sq, float weight, bool first,
                                     const DzChannel &ch, unsigned switches, hipStream_t stream);

// ---- drizzle.hip ----
// nl_stack_frame_drizzle_from's kernel: the rows [row0, row0 + rows) of a dst_w wide output grid; sum / wgt = the two
// planes of those rows; point = NL_DZ_POINT; switches: kProjDirectOnly of project.hpp
hipError_t launch_drizzle(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0, int rows,
                          const DzGeom &geom, float weight, bool first, bool point, unsigned switches, hipStream_t stream);
// how many tiles of that launch stage their candidate box in LDS, how many read global memory (host arithmetic)
void drizzle_tile_paths(const float *src, int src_w, int src_h, int dst_w, int row0, int rows, const DzGeom &geom,
                        unsigned switches, int64_t *staged, int64_t *direct);
// out[i] = wgt[i] > min_weight ? sum[i] / wgt[i] : empty (any aliasing)
hipError_t launch_drizzle_finalize(const float *sum, const float *wgt, float *out, int64_t n, float min_weight, float empty,
                                   hipStream_t stream);
// nl_stack_frame_reject_against's kernel over n pixels on `blocks` workgroups: counts[2 * b] / [2 * b + 1] = the
// pixels workgroup b took out low / high
hipError_t launch_reject_against(float *frame, const float *model, int64_t n, float low, float high,
                                 unsigned long long *counts, int blocks, hipStream_t stream);

}  // namespace nl
