// drizzle_square.hip -- the square drizzle kernel: the exact overlap of a source pixel's drop, a parallelogram under the
// transform (a rotated square for a similarity), with an output pixel, for nl_stack_frame_drizzle_square_from and
// nl_stack_frame_drizzle_square_cfa_from.  AN EXTENSION: include/nlstack_sqdrizzle.h carries the definition these
// kernels compute bit for bit.
//
// A third candidate-weight function in the walks of drizzle_walk.hpp, in a unit of its own so that the instantiations of
// drizzle.hip and drizzle_cfa.hip keep their code (DESIGN.md sections 6u / 6v).  The tile shape, the candidate box (with
// the square R), its staging, the NaN weight of a candidate that is none and the strided CFA walks are theirs.
//
// A candidate: the bounding box of the drop against the pixel first (NL_DZ_TURBO's two clamps with the box's half-sides),
// then the four corners of the drop relative to the pixel, the pixel being the unit square, and the sum of the signed
// areas between each edge and the x-axis inside the unit square (the sgarea / boxer scheme).  dz_edge computes every
// path of the definition and selects: a value of a path not taken (a division by zero among them) is discarded.
//
// Most candidates of a window fail the bounding-box test, and an edge costs three IEEE divisions.  The four edges of a
// candidate are skipped where no lane of the wave passed the test (one ballot, a branch that is uniform over the wave; a
// lane that failed carries its NaN weight either way, so no bit moves).  Bit 3 of the flags evaluates them for every
// candidate, the plain form, kept behind developer switch 262144 as the yardstick of the skip.
//
// Bit-exact: operands in the header's order, no FMA (-ffp-contract=off), IEEE division.
#include <math.h>

#include "drizzle.hpp"
#include "drizzle_walk.hpp"
#include "launch_common.hpp"

namespace nl {

namespace {

// NL_DZ_TURBO's overlap of [centre - half, centre + half] with [pix - 0.5, pix + 0.5]
__device__ __forceinline__ float dz_box_overlap(float centre, float half, float pix)
{
    float lo = centre - half, e = pix - 0.5f;
    if (e > lo) lo = e;
    float hi = centre + half;
    e = pix + 0.5f;
    if (e < hi) hi = e;
    return hi - lo;
}

// the header's edge(x1, y1, x2, y2): the signed area between the segment and the x-axis inside the unit square
__device__ __forceinline__ float dz_edge(float x1, float y1, float x2, float y2)
{
    const float dx = x2 - x1, dy = y2 - y1;
    const bool back = dx < 0.0f;
    float xlo = back ? x2 : x1, xhi = back ? x1 : x2;
    const bool none = dx == 0.0f || xlo >= 1.0f || xhi <= 0.0f;
    xlo = xlo < 0.0f ? 0.0f : xlo;
    xhi = xhi > 1.0f ? 1.0f : xhi;
    const float m = dy / dx, c = y1 - m * x1;
    float ylo = m * xlo + c, yhi = m * xhi + c;
    const bool below = ylo <= 0.0f && yhi <= 0.0f, above = ylo >= 1.0f && yhi >= 1.0f;
    const float sg = back ? -1.0f : 1.0f;
    const float whole = sg * (xhi - xlo);
    const float det = x1 * y2 - y1 * x2;
    const float x_axis = det / dy;
    if (ylo < 0.0f) { ylo = 0.0f; xlo = x_axis; }
    if (yhi < 0.0f) { yhi = 0.0f; xhi = x_axis; }
    const float xtop = (dx + det) / dy;
    const float inside = sg * ((0.5f * (xhi - xlo)) * (yhi + ylo));
    const float leaves = sg * ((0.5f * (xtop - xlo)) * (1.0f + ylo) + (xhi - xtop));
    const float enters = sg * ((0.5f * (xhi - xtop)) * (1.0f + yhi) + (xtop - xlo));
    const float part = ylo <= 1.0f ? (yhi <= 1.0f ? inside : leaves) : enters;
    return none || below ? 0.0f : (above ? whole : part);
}

// a kernel argument as a vector register: F and the ten values of DzSquare beside G, the tile's loop state and an
// edge's comparisons are more scalar registers than a wave has, and the compiler spills them rather than these
__device__ __forceinline__ float dz_in_vgpr(float x)
{
    float v;
    asm volatile("v_mov_b32 %0, %1" : "=v"(v) : "s"(x));
    return v;
}

__device__ __forceinline__ int dz_in_vgpr(int x) { return __float_as_int(dz_in_vgpr(__int_as_float(x))); }

struct DzSquareDrop {
    ProjInv f;                         // DzGeom's F and DzSquare, in vector registers
    float cx[4], cy[4], bx, by;
    float weight;
    bool every;                        // the edges of every candidate (uniform)
    __device__ __forceinline__ DzSquareDrop(const DzGeom &q, const DzSquare &sq, float w, bool all)
        : f{dz_in_vgpr(q.f.a), dz_in_vgpr(q.f.b), dz_in_vgpr(q.f.c), dz_in_vgpr(q.f.d), dz_in_vgpr(q.f.e), dz_in_vgpr(q.f.f)},
          bx(dz_in_vgpr(sq.bx)), by(dz_in_vgpr(sq.by)), weight(dz_in_vgpr(w)), every(all)
    {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cx[k] = dz_in_vgpr(sq.cx[k]);
            cy[k] = dz_in_vgpr(sq.cy[k]);
        }
    }
    __device__ __forceinline__ float operator()(float fi, float fj, float px, float py, bool &ok) const
    {
        const float u = proj_x(f, fi, fj), vv = proj_y(f, fi, fj);
        const float ox = dz_box_overlap(u, bx, px), oy = dz_box_overlap(vv, by, py);
        // ok leaves as "inside the drop's bounding box": the walk reads such a candidate's pixel whether or not its
        // area is positive, and the NaN weight drops it.  The test goes into the weight at once (NaN * ar is NaN), so
        // that no lane mask lives through the edges: (2R + 1)^2 of them spill SGPRs.
        ok = ok && ox > 0.0f && oy > 0.0f;
        const float nan = __builtin_nanf("");
        // (uniform over the wave.  The branch is there in the plain form too, always taken: it keeps the edges of one
        // candidate in a basic block of their own.  As straight-line code the compiler interleaves the edges of the
        // whole window and needs 348 to 512 VGPRs and scratch.)
        if (!every && __builtin_amdgcn_ballot_w64(ok) == 0) return nan;
        const float gate = ok ? weight : nan;
        const float ux = u - px, vy = vv - py;
        float x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            x[k] = (ux + cx[k]) + 0.5f;
            y[k] = (vy + cy[k]) + 0.5f;
        }
        const float ar = ((dz_edge(x[0], y[0], x[1], y[1]) + dz_edge(x[1], y[1], x[2], y[2])) + dz_edge(x[2], y[2], x[3], y[3])) +
                         dz_edge(x[3], y[3], x[0], y[0]);
        return ar > 0.0f ? gate * ar : nan;
    }
};

// flags: drizzle_walk.hpp's drizzle_tile, and bit 3 = the edges of every candidate
template <int R>
__global__ __launch_bounds__(256) void drizzle_square_tile_kernel(const float *__restrict__ src, int src_w, int src_h,
                                                                  float *__restrict__ sum, float *__restrict__ wgt, int dst_w,
                                                                  int row0, int rows, DzGeom q, DzSquare sq, float weight,
                                                                  unsigned flags)
{
    __shared__ float lds[kDzLdsFloats];
    drizzle_tile<R>(lds, src, src_w, src_h, sum, wgt, dst_w, row0, rows, q.g, DzSquareDrop(q, sq, weight, flags & 8u), flags);
}

template <int R, bool GREEN>
__global__ __launch_bounds__(256) void drizzle_square_cfa_tile_kernel(const float *__restrict__ src, int src_w, int src_h,
                                                                      float *__restrict__ sum, float *__restrict__ wgt,
                                                                      int dst_w, int row0, int rows, DzGeom q, DzSquare sq,
                                                                      float weight, unsigned flags, DzChannel ch)
{
    __shared__ float lds[kDzLdsFloats];
    const DzChannel chv = {dz_in_vgpr(ch.xo), dz_in_vgpr(ch.yo), ch.green, dz_in_vgpr(ch.par_x), dz_in_vgpr(ch.par_y)};
    drizzle_cfa_tile<R, DzSquareDrop, GREEN>(lds, src, src_w, src_h, sum, wgt, dst_w, row0, rows, q.g,
                                             DzSquareDrop(q, sq, weight, flags & 8u), flags, chv);
}

// bits 2 / 3 of the kernels' flags
unsigned square_flags(bool first, unsigned switches)
{
    return (first ? 4u : 0u) | ((switches & kDzSquareEveryCandidate) ? 8u : 0u);
}

}  // namespace

hipError_t launch_drizzle_square(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0,
                                 int rows, const DzGeom &geom, const DzSquare &sq, float weight, bool first,
                                 unsigned switches, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + kProjTileW - 1) / kProjTileW), (unsigned)((rows + kProjTileH - 1) / kProjTileH));
    const unsigned flags = dz_tile_flags(src, src_w, switches) | square_flags(first, switches);
    Launcher L(stream);
    with_class<1, 2, 3>(geom.radius, [&](auto R) {
        L(drizzle_square_tile_kernel<decltype(R)::value>, grid, 256, 0, src, src_w, src_h, sum, wgt, dst_w, row0, rows, geom, sq,
          weight, flags);
    });
    return L.err;
}

hipError_t launch_drizzle_square_cfa(const float *src, int src_w, int src_h, float *sum, float *wgt, int dst_w, int row0,
                                     int rows, const DzGeom &geom, const DzSquare &sq, float weight, bool first,
                                     const DzChannel &ch, unsigned switches, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + kProjTileW - 1) / kProjTileW), (unsigned)((rows + kProjTileH - 1) / kProjTileH));
    const unsigned flags = dz_tile_flags(src, src_w, switches) | square_flags(first, switches);
    Launcher L(stream);
    with_class<1, 2, 3>(geom.radius, [&](auto R) {
        with_bool(ch.green != 0, [&](auto G) {
            L(drizzle_square_cfa_tile_kernel<decltype(R)::value, decltype(G)::value>, grid, 256, 0, src, src_w, src_h, sum, wgt,
              dst_w, row0, rows, geom, sq, weight, flags, ch);
        });
    });
    return L.err;
}

}  // namespace nl
