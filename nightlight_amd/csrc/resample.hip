// resample.hip -- the resident projection of project.hip with a wider resampling kernel: bicubic (Catmull-Rom, radius 2)
// and Lanczos-3 (radius 3, weights from a 1024-phase table), optionally clamped to the four central taps, for
// nl_stack_frame_resample_from / nl_group_frame_resample_from.  AN EXTENSION: the reference's Image.Project resamples
// bilinearly; include/nlstack_resample.h carries the definition these kernels compute bit for bit (given the table).
//
// The structure is project.hip's.  A workgroup owns a kProjTileW x kProjTileH tile of the destination; wave w makes
// rows w, w + 4, ... of it, lane l the columns l, l + 64, l + 128, l + 192 of a row, so every store instruction of a
// wave covers 256 contiguous bytes and a lane has four independent pixels in flight.  From the four corners of its
// tile (project.hpp) the workgroup computes the source box of the tile, grown by R - 1 pixels on every side and
// clipped to the source; it stages the box in LDS (each source byte fetched once, 16 bytes per lane where the source's
// width allows) when the box is within kRsLdsFloats, else every tap comes from global memory.
//
// Per pixel there are three cases (the header's): out of bounds; the 2x2 footprint fits but the wide one does not --
// the bilinear value, project.hip's arithmetic on the four central taps, which the same box holds; the wide footprint
// fits -- the separable sum.  No case branches around its loads: a pixel that has no wide footprint reads its (2R)^2
// taps from one place that is always there (strides 0) and drops the sum, a pixel out of bounds reads element 0.
//
// The Lanczos-3 table (24 KiB) stays in global memory and its rows are gathered through the vector cache: the lanes of
// a wave have different x phases, so an LDS copy would be gathered just the same, and it would take the LDS of three
// more resident workgroups per CU.  The y phase is the same for a whole row under a pure shift: one row, broadcast.
//
// Bit-exact: coordinates, floor and range tests as project.hip; every sum left to right, no FMA (-ffp-contract=off).
#include <math.h>

#include <mutex>
#include <vector>

#include "dev_memory.hpp"
#include "launch_common.hpp"
#include "project.hpp"

namespace nl {

namespace {

constexpr int kRsLdsFloats = 10240;       // 40 KiB: four workgroups (16 waves) share a CU's 160 KiB
constexpr int kRsMaxDevices = 64;

// the weights of the 2R taps along one axis at fraction t in [0, 1)
template <int R>
__device__ __forceinline__ void rs_weights(float t, const float *__restrict__ table, float (&w)[2 * R])
{
    if constexpr (R == 2) {                                                  // Keys, a = -0.5, Horner
        w[0] = ((-0.5f * t + 1.0f) * t - 0.5f) * t;
        w[1] = (1.5f * t - 2.5f) * t * t + 1.0f;
        w[2] = ((-1.5f * t + 2.0f) * t + 0.5f) * t;
        w[3] = (0.5f * t - 0.5f) * t * t;
    } else {                                                                 // row (int)(t * 1024) of the table
        const int q = (int)(t * (float)NL_RS_PHASES);                        // (exact product, q <= 1023)
        const float2 *row = reinterpret_cast<const float2 *>(table + 6 * q); // rows are 24 bytes: 8-byte aligned
        const float2 a = row[0], b = row[1], c = row[2];
        w[0] = a.x; w[1] = a.y; w[2] = b.x; w[3] = b.y; w[4] = c.x; w[5] = c.y;
    }
}

// rows of the tile for this wave, four pixels per lane and row.  mem = the box in LDS (origin b.x0, b.y0, pitch
// b.pitch) or the source itself (origin 0, 0, pitch src_w).
template <int R, bool CLAMP, bool NT, class Index>
__device__ __forceinline__ void resample_rows(const float *__restrict__ mem, int org_x, int org_y, Index pitch, int src_w,
                                              int src_h, float *__restrict__ dst, int dst_w, int row0, int c0, int r_first,
                                              int r_end, const ProjInv &t, float oob, const float *__restrict__ table)
{
    const int lane = threadIdx.x & 63;
    for (int r = r_first + (int)(threadIdx.x >> 6); r < r_end; r += 4) {
        const float py = (float)(row0 + r);
        float wx[4][2 * R], wy[4][2 * R], xr[4], yr[4];
        Index at[4], sx[4], sy[4], dx[4], dy[4];
        bool ok[4], wide[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int col = c0 + lane + 64 * j;
            const float px = (float)col;
            const float X = proj_x(t, px, py);                               // coord.go:142 (left to right)
            const float Y = proj_y(t, px, py);                               // coord.go:143
            const float fx = floorf(X), fy = floorf(Y);                      // project.go:52
            // (project.hip: NaN and out-of-range coordinates are out of bounds; so is a column beyond the destination)
            ok[j] = col < dst_w && fx >= 0.0f && fy >= 0.0f && fx < 2147483520.0f && fy < 2147483520.0f;
            int xl = 0, yl = 0;
            if (ok[j]) {
                xl = (int)fx; yl = (int)fy;
                ok[j] = (int64_t)xl + 1 < src_w && (int64_t)yl + 1 < src_h;
            }
            xr[j] = X - (float)xl; yr[j] = Y - (float)yl;                    // project.go:54
            wide[j] = ok[j] && xl - (R - 1) >= 0 && xl + R <= src_w - 1 && yl - (R - 1) >= 0 && yl + R <= src_h - 1;
            at[j] = ok[j] ? (Index)(yl - org_y) * pitch + (Index)(xl - org_x) : 0;
            dx[j] = ok[j] ? 1 : 0; dy[j] = ok[j] ? pitch : 0;
            sx[j] = wide[j] ? 1 : 0; sy[j] = wide[j] ? pitch : 0;
            rs_weights<R>(wide[j] ? xr[j] : 0.0f, table, wx[j]);
            rs_weights<R>(wide[j] ? yr[j] : 0.0f, table, wy[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int col = c0 + lane + 64 * j;
            // the four central taps: the bilinear value (project.go:68-70) and the clamp's range
            const float t00 = mem[at[j]], t01 = mem[at[j] + dx[j]], t10 = mem[at[j] + dy[j]], t11 = mem[at[j] + dy[j] + dx[j]];
            const float omx = 1.0f - xr[j], omy = 1.0f - yr[j];
            const float vyl = t00 * omx + t01 * xr[j];
            const float vyh = t10 * omx + t11 * xr[j];
            const float vb = vyl * omy + vyh * yr[j];
            // the separable sum over the wide footprint, rows first
            float v = 0.0f;
#pragma unroll
            for (int a = 0; a < 2 * R; a++) {
                const Index p = at[j] + (Index)(a - (R - 1)) * sy[j];
                float ra = mem[p - (R - 1) * sx[j]] * wx[j][0];
#pragma unroll
                for (int i = 1; i < 2 * R; i++) ra = ra + mem[p + (Index)(i - (R - 1)) * sx[j]] * wx[j][i];
                v = a == 0 ? ra * wy[j][0] : v + ra * wy[j][a];
            }
            if constexpr (CLAMP) {
                float lo = t00, hi = t00;
                if (t01 < lo) lo = t01;
                if (t10 < lo) lo = t10;
                if (t11 < lo) lo = t11;
                if (t01 > hi) hi = t01;
                if (t10 > hi) hi = t10;
                if (t11 > hi) hi = t11;
                if (v < lo) v = lo;
                if (v > hi) v = hi;
            }
            if (!wide[j]) v = vb;
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
template <int R, bool CLAMP, bool NT>
__global__ __launch_bounds__(256) void resample_tile_kernel(const float *__restrict__ src, int src_w, int src_h,
                                                            float *__restrict__ dst, int dst_w, int row0, int rows,
                                                            ProjInv t, float oob, const float *__restrict__ table,
                                                            unsigned flags)
{
    __shared__ float lds[kRsLdsFloats];
    const int c0 = blockIdx.x * kProjTileW, r0 = blockIdx.y * kProjTileH;
    const int c1 = min(c0 + kProjTileW, dst_w) - 1, r_end = min(r0 + kProjTileH, rows);
    const bool vec = flags & 1u;
    ProjBox b = {0, 0, 0, 0, 0};
    const bool staged = (flags & 2u) && proj_tile_box(t, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, vec, b, R - 1,
                                                      kRsLdsFloats);
    if (staged) {                                                            // (uniform over the workgroup)
        if (vec) stage_box<true>(src, src_w, b, lds);
        else stage_box<false>(src, src_w, b, lds);
        __syncthreads();
        resample_rows<R, CLAMP, NT, int>(lds, b.x0, b.y0, b.pitch, src_w, src_h, dst, dst_w, row0, c0, r0, r_end, t, oob, table);
    } else {
        resample_rows<R, CLAMP, NT, int64_t>(src, 0, 0, src_w, src_w, src_h, dst, dst_w, row0, c0, r0, r_end, t, oob, table);
    }
}

// bits 0 / 1 of the kernel's flags (project.hip's rule)
unsigned tile_flags(const float *src, int src_w, const float inv[6], unsigned switches)
{
    bool finite = true;
    for (int i = 0; i < 6; i++) finite = finite && isfinite(inv[i]);
    const bool vec = (src_w & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    return (vec ? 1u : 0u) | (!(switches & kProjDirectOnly) && finite ? 2u : 0u);
}

// L(x) = 3 sin(pi x) sin(pi x / 3) / (pi^2 x^2) of the header, in double
double lanczos3(double x)
{
    if (x == 0.0) return 1.0;
    if (x == floor(x)) return 0.0;
    return 3.0 * sin(M_PI * x) * sin(M_PI * x / 3.0) / (M_PI * M_PI * x * x);
}

}  // namespace

const float *lanczos3_table_host()
{
    static const std::vector<float> table = [] {
        std::vector<float> t(NL_RS_PHASES * 6);
        for (int q = 0; q < NL_RS_PHASES; q++) {
            double w[6], sum = 0.0;
            for (int i = 0; i < 6; i++) sum += w[i] = lanczos3((double)q / NL_RS_PHASES - (double)(i - 2));
            for (int i = 0; i < 6; i++) t[6 * q + i] = (float)(w[i] / sum);
        }
        return t;
    }();
    return table.data();
}

hipError_t lanczos3_table_device(int device, const float **table)
{
    static std::mutex mu;
    static float *copies[kRsMaxDevices] = {};
    if (device < 0 || device >= kRsMaxDevices) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> hold(mu);
    if (!copies[device]) {
        const size_t bytes = sizeof(float) * NL_RS_PHASES * 6;
        float *d = nullptr;
        hipError_t e = dev_malloc(&d, bytes);
        if (e != hipSuccess) return e;
        if ((e = hipMemcpy(d, lanczos3_table_host(), bytes, hipMemcpyHostToDevice)) != hipSuccess) {
            (void)hipFree(d);
            return e;
        }
        copies[device] = d;
    }
    *table = copies[device];
    return hipSuccess;
}

hipError_t launch_resample_tiled(const float *src, int src_w, int src_h, float *dst, int dst_w, int row0, int rows,
                                 const float inv[6], float oob, int radius, bool clamp, const float *table,
                                 unsigned switches, hipStream_t stream)
{
    const dim3 grid((unsigned)((dst_w + kProjTileW - 1) / kProjTileW), (unsigned)((rows + kProjTileH - 1) / kProjTileH));
    const ProjInv t = {inv[0], inv[1], inv[2], inv[3], inv[4], inv[5]};
    const unsigned flags = tile_flags(src, src_w, inv, switches);
    Launcher L(stream);
    with_bool(radius == 3, [&](auto L3) {
        with_bool(clamp, [&](auto C) {
            with_bool(!(switches & kProjPlainStores), [&](auto N) {
                L(resample_tile_kernel<decltype(L3)::value ? 3 : 2, decltype(C)::value, decltype(N)::value>, grid, 256, 0,
                  src, src_w, src_h, dst, dst_w, row0, rows, t, oob, table, flags);
            });
        });
    });
    return L.err;
}

void resample_tile_paths(const float *src, int src_w, int src_h, int dst_w, int row0, int rows, const float inv[6],
                         int radius, unsigned switches, int64_t *staged, int64_t *direct)
{
    const unsigned flags = tile_flags(src, src_w, inv, switches);
    const ProjInv t = {inv[0], inv[1], inv[2], inv[3], inv[4], inv[5]};
    int64_t n_staged = 0, n_direct = 0;
    for (int r0 = 0; r0 < rows; r0 += kProjTileH)
        for (int c0 = 0; c0 < dst_w; c0 += kProjTileW) {
            const int c1 = (c0 + kProjTileW < dst_w ? c0 + kProjTileW : dst_w) - 1;
            const int r_end = r0 + kProjTileH < rows ? r0 + kProjTileH : rows;
            ProjBox b;
            if ((flags & 2u) && proj_tile_box(t, src_w, src_h, c0, c1, row0 + r0, row0 + r_end - 1, flags & 1u, b, radius - 1,
                                              kRsLdsFloats))
                n_staged++;
            else
                n_direct++;
        }
    *staged = n_staged;
    *direct = n_direct;
}

}  // namespace nl
