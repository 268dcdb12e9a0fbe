// project.hpp -- the tile geometry of project.hip and resample.hip (the same projection with a wider resampling kernel),
// the one piece of arithmetic their kernels and the host share: the source box of a destination tile, and how a
// workgroup stages that box in LDS.  Host and device run the same fp32 operations (no contraction on either side), so
// project_tile_paths() and resample_tile_paths() count exactly the tiles the kernels stage.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace nl {

constexpr int kProjTileW = 256;           // destination columns of a workgroup's tile: 64 lanes x 4 pixels
constexpr int kProjTileH = 16;            // destination rows: 4 waves x 4 rows
constexpr int kProjLdsFloats = 6144;      // 24 KiB: six workgroups share a CU's 160 KiB
// switches of launch_project (developer switches 32768 / 65536 of nl_stack_set_dev_flags)
constexpr unsigned kProjDirectOnly = 1u;  // no tile stages its box: every tap from global memory
constexpr unsigned kProjPlainStores = 2u; // plain instead of nontemporal result stores

// the inverse transform as the kernel takes it
struct ProjInv { float a, b, c, d, e, f; };

// coord.go:142-143, left to right: the coordinates of destination pixel (col, row) in the source
__host__ __device__ inline float proj_x(const ProjInv &t, float px, float py) { return t.a * px + t.b * py + t.c; }
__host__ __device__ inline float proj_y(const ProjInv &t, float px, float py) { return t.d * px + t.e * py + t.f; }

// rows [y0, y0 + h) x columns [x0, x0 + w) of the source; in LDS row y of it starts at float (y - y0) * pitch
struct ProjBox { int x0, y0, w, h, pitch; };

// floor(v) as an int where it matters: anything below -1 is -1, anything above 2^30 is 2^30 (v is no NaN)
__host__ __device__ inline int proj_floor_clamped(float v)
{
    const float f = floorf(v);
    return (int)(f < -1.0f ? -1.0f : (f > 1073741824.0f ? 1073741824.0f : f));
}

// The source box of the destination tile of columns [c0, c1] and image rows [r0, r1] (inclusive): every source pixel
// that a pixel of the tile with its whole 2x2 footprint inside the source can tap.  False when the tile takes its
// taps from global memory instead: a coordinate that is NaN at a corner, a box beyond the LDS budget, or no pixel of
// the tile in bounds at all (then nothing is read either way).
//
// Why the four corners are enough, with no margin: X = fl(fl(fl(a*px) + fl(b*py)) + c) is what every pixel computes.
// Rounding is monotone, so for a fixed py X is monotone in px (rising or falling with the sign of a, whatever py is),
// and for a fixed px monotone in py.  The smallest and the largest X over the rectangle -- the computed ones, rounding
// included -- are therefore taken at corners, and floor(X), floor(X) + 1 of every pixel lie in
// [floor(min corner), floor(max corner) + 1].  Same for Y.  With finite coefficients a NaN (inf - inf) inside the
// rectangle implies one at a corner by the same argument; the launcher stages nothing when a coefficient is not finite.
//
// grow (resample.hip: R - 1 of a kernel of radius R) widens the box by that many pixels on every side, as far as the
// source reaches: the wide footprints of the same pixels.  Whether a tile has a pixel in bounds does not depend on it.
// lds_floats is the budget of the kernel that asks.
__host__ __device__ inline bool proj_tile_box(const ProjInv &t, int src_w, int src_h, int c0, int c1, int r0, int r1,
                                              bool vec, ProjBox &b, int grow = 0, int lds_floats = kProjLdsFloats)
{
    const float px0 = (float)c0, px1 = (float)c1, py0 = (float)r0, py1 = (float)r1;
    const float x00 = proj_x(t, px0, py0), x10 = proj_x(t, px1, py0), x01 = proj_x(t, px0, py1), x11 = proj_x(t, px1, py1);
    const float y00 = proj_y(t, px0, py0), y10 = proj_y(t, px1, py0), y01 = proj_y(t, px0, py1), y11 = proj_y(t, px1, py1);
    if (x00 != x00 || x10 != x10 || x01 != x01 || x11 != x11 || y00 != y00 || y10 != y10 || y01 != y01 || y11 != y11)
        return false;
    const float xmin = fminf(fminf(x00, x10), fminf(x01, x11)), xmax = fmaxf(fmaxf(x00, x10), fmaxf(x01, x11));
    const float ymin = fminf(fminf(y00, y10), fminf(y01, y11)), ymax = fmaxf(fmaxf(y00, y10), fmaxf(y01, y11));
    int x0 = proj_floor_clamped(xmin), x1 = proj_floor_clamped(xmax) + 1;
    int y0 = proj_floor_clamped(ymin), y1 = proj_floor_clamped(ymax) + 1;
    // a pixel in bounds has 0 <= xl and xl + 1 <= src_w - 1 (ingest: project.go:56), so the box ends at the source's edges
    if (x0 < 0) x0 = 0;
    if (y0 < 0) y0 = 0;
    if (x1 > src_w - 1) x1 = src_w - 1;
    if (y1 > src_h - 1) y1 = src_h - 1;
    if (x1 - x0 < 1 || y1 - y0 < 1) return false;          // no room for one 2x2 footprint
    x0 = x0 - grow < 0 ? 0 : x0 - grow;
    y0 = y0 - grow < 0 ? 0 : y0 - grow;
    x1 = x1 + grow > src_w - 1 ? src_w - 1 : x1 + grow;
    y1 = y1 + grow > src_h - 1 ? src_h - 1 : y1 + grow;
    if (vec) {                                             // whole 16-byte groups of a row (src_w is a multiple of 4)
        x0 &= ~3;
        x1 |= 3;
    }
    b.x0 = x0;
    b.y0 = y0;
    b.w = x1 - x0 + 1;
    b.h = y1 - y0 + 1;
    b.pitch = b.w | 1;                                     // odd: taps down a column (a 90 degree turn) spread over the banks
    return (int64_t)b.pitch * b.h <= lds_floats;
}

// the box of the tile into LDS: unit = 4 floats (16-byte loads) or 1; at most kProjLdsFloats / 256 units per lane in
// flight per round
template <bool VEC>
__device__ __forceinline__ void stage_box(const float *__restrict__ src, int src_w, const ProjBox &b, float *lds)
{
    constexpr int U = VEC ? 6 : 8;
    const int per_row = VEC ? b.w >> 2 : b.w;
    const int total = per_row * b.h;
    const float *base = src + (int64_t)b.y0 * src_w + b.x0;
    for (int first = threadIdx.x; first < total; first += 256 * U) {
        float4 v[U];
        int at[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int i = first + 256 * u;
            at[u] = -1;
            if (i < total) {
                const int y = i / per_row, x = i - y * per_row;
                if constexpr (VEC) {
                    v[u] = *reinterpret_cast<const float4 *>(base + (int64_t)y * src_w + 4 * x);
                    at[u] = y * b.pitch + 4 * x;
                } else {
                    v[u].x = base[(int64_t)y * src_w + x];
                    at[u] = y * b.pitch + x;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            if (at[u] < 0) continue;
            lds[at[u]] = v[u].x;
            if constexpr (VEC) {
                lds[at[u] + 1] = v[u].y; lds[at[u] + 2] = v[u].z; lds[at[u] + 3] = v[u].w;
            }
        }
    }
}

}  // namespace nl
