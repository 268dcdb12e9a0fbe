// project.hip -- Image.Project (internal/fits/project.go:26-76): bilinear resampling of a source frame through the
// inverted Transform2D (internal/star/coord.go:141-145, 159-199) into the rows [row0, row0 + rows) of a destination,
// out of bounds -> the given value (NaN in the pipeline), for nl_stack_frame_project_from / nl_group_frame_project_from
// (source = a resident slot).  The projected uploads, whose frame has just crossed PCIe, keep project_kernel of
// ingest.hip until this kernel has been timed against it: the dispatch rule is that one line.
//
// A workgroup owns a kProjTileW x kProjTileH tile of the destination.  Wave w makes rows w, w + 4, ... of it, lane l the
// columns l, l + 64, l + 128, l + 192 of a row: every load and store instruction of a wave covers 256 contiguous bytes,
// and the sixteen taps of a lane's four pixels are independent and in flight together.  Per workgroup, from the four
// corners of its tile (project.hpp: exact, no margin), the source box of the tile is either staged in LDS -- each source
// byte fetched once, 16 bytes per lane where the source's width allows -- and the taps come from there, or, when the box
// is beyond the LDS budget (strong scale changes), the taps come from global memory as in project_kernel.
//
// Bit-exact: per pixel the coordinates, floor and range tests, the three lerps and their operand order are those of
// the reference (no FMA: -ffp-contract=off); only where a tap is read from differs.
#include <math.h>

#include "launch_common.hpp"
#include "project.hpp"

namespace nl {

namespace {

// rows of the tile for this wave, four pixels per lane and row.  STAGED: taps from the box in LDS, else from src.
// A pixel out of bounds taps element 0 (always there) and drops the result: no branch around the loads.
template <bool NT, bool STAGED>
__device__ __forceinline__ void project_rows(const float *__restrict__ src, int src_w, int src_h, float *__restrict__ dst,
                                             int dst_w, int row0, int c0, int r_first, int r_end, const ProjInv &t,
                                             float oob, const ProjBox &b, const float *lds)
{
    const int lane = threadIdx.x & 63;
    for (int r = r_first + (int)(threadIdx.x >> 6); r < r_end; r += 4) {
        const float py = (float)(row0 + r);
        float tap[4][4], xr[4], yr[4];
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int col = c0 + lane + 64 * j;
            const float px = (float)col;
            const float X = proj_x(t, px, py);                               // coord.go:142 (left to right)
            const float Y = proj_y(t, px, py);                               // coord.go:143
            const float fx = floorf(X), fy = floorf(Y);                      // project.go:52
            // int32(math.Floor(x)) of NaN / out-of-range is negative on amd64 => out of bounds (project.go:56)
            // (a column beyond the destination is made and dropped: it taps nothing, the box does not cover it)
            ok[j] = col < dst_w && fx >= 0.0f && fy >= 0.0f && fx < 2147483520.0f && fy < 2147483520.0f;
            int xl = 0, yl = 0;
            if (ok[j]) {
                xl = (int)fx; yl = (int)fy;
                ok[j] = (int64_t)xl + 1 < src_w && (int64_t)yl + 1 < src_h;
            }
            xr[j] = X - (float)xl; yr[j] = Y - (float)yl;                    // project.go:54
            if constexpr (STAGED) {
                const int p = ok[j] ? (yl - b.y0) * b.pitch + (xl - b.x0) : 0;
                const int dx = ok[j] ? 1 : 0, dy = ok[j] ? b.pitch : 0;
                tap[j][0] = lds[p]; tap[j][1] = lds[p + dx]; tap[j][2] = lds[p + dy]; tap[j][3] = lds[p + dy + dx];
            } else {
                const int64_t p = ok[j] ? (int64_t)xl + (int64_t)yl * src_w : 0;
                const int64_t dx = ok[j] ? 1 : 0, dy = ok[j] ? src_w : 0;
                tap[j][0] = src[p]; tap[j][1] = src[p + dx]; tap[j][2] = src[p + dy]; tap[j][3] = src[p + dy + dx];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int col = c0 + lane + 64 * j;
            const float omx = 1.0f - xr[j], omy = 1.0f - yr[j];
            const float vyl = tap[j][0] * omx + tap[j][1] * xr[j];          // project.go:68
            const float vyh = tap[j][2] * omx + tap[j][3] * xr[j];
            float v = vyl * omy + vyh * yr[j];                               // project.go:70
            if (!ok[j]) v = oob;
            if (col < dst_w) {
                float *q = dst + (int64_t)r * dst_w + col;
                if (NT) __builtin_nontemporal_store(v, q);
                else *q = v;
            }
        }
    }
}

// flags: bit 0 = the source allows 16-byte loads, bit 1 = tiles may stage their box
template <bool NT>
__global__ __launch_bounds__(256) void project_tile_kernel(const float *__restrict__ src, int src_w, int src_h,
                                                           float *__restrict__ dst, int dst_w, int row0, int rows,
                                                           ProjInv t, float oob, unsigned flags)
{
    __shared__ float lds[kProjLdsFloats];
    const int c0 = blockIdx.x * kProjTileW, r0 = blockIdx.y * kProjTileH;
    const int c1 = min(c0 + kProjTileW, dst_w) - 1, r_end = min(r0 + kProjTileH, rows);
    const bool vec = flags & 1u;
    ProjBox b = {0, 0, 0, 0, 0};
    const bool staged = (flags & 2u) && proj_tile_box(t, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, vec, b);
    if (staged) {                                                            // (uniform over the workgroup)
        if (vec) stage_box<true>(src, src_w, b, lds);
        else stage_box<false>(src, src_w, b, lds);
        __syncthreads();
        project_rows<NT, true>(src, src_w, src_h, dst, dst_w, row0, c0, r0, r_end, t, oob, b, lds);
    } else {
        project_rows<NT, false>(src, src_w, src_h, dst, dst_w, row0, c0, r0, r_end, t, oob, b, lds);
    }
}

bool all_finite(const float inv[6])
{
    for (int i = 0; i < 6; i++)
        if (!isfinite(inv[i])) return false;
    return true;
}

// bits 0 / 1 of the kernel's flags
unsigned tile_flags(const float *src, int src_w, const float inv[6], unsigned switches)
{
    const bool vec = (src_w & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    const bool stage = !(switches & kProjDirectOnly) && all_finite(inv);
    return (vec ? 1u : 0u) | (stage ? 2u : 0u);
}

}  // namespace

hipError_t launch_project_tiled(const float *src, int src_w, int src_h, float *dst, int dst_w, int row0, int rows,
                                const float inv[6], float oob, unsigned switches, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + kProjTileW - 1) / kProjTileW), (unsigned)((rows + kProjTileH - 1) / kProjTileH));
    const ProjInv t = {inv[0], inv[1], inv[2], inv[3], inv[4], inv[5]};
    const unsigned flags = tile_flags(src, src_w, inv, switches);
    Launcher L(stream);
    with_bool(!(switches & kProjPlainStores), [&](auto N) {
        L(project_tile_kernel<decltype(N)::value>, grid, 256, 0, src, src_w, src_h, dst, dst_w, row0, rows, t, oob, flags);
    });
    return L.err;
}

void project_tile_paths(const float *src, int src_w, int src_h, int dst_w, int row0, int rows, const float inv[6],
                        unsigned switches, int64_t *staged, int64_t *direct)
{
    const unsigned flags = tile_flags(src, src_w, inv, switches);
    const ProjInv t = {inv[0], inv[1], inv[2], inv[3], inv[4], inv[5]};
    int64_t n_staged = 0, n_direct = 0;
    for (int r0 = 0; r0 < rows; r0 += kProjTileH)
        for (int c0 = 0; c0 < dst_w; c0 += kProjTileW) {
            const int c1 = (c0 + kProjTileW < dst_w ? c0 + kProjTileW : dst_w) - 1;
            const int r_end = r0 + kProjTileH < rows ? r0 + kProjTileH : rows;
            ProjBox b;
            if ((flags & 2u) && proj_tile_box(t, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, flags & 1u, b)) n_staged++;
            else n_direct++;
        }
    *staged = n_staged;
    *direct = n_direct;
}

}  // namespace nl
