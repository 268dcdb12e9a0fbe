// stack_coverage.hip -- the coverage map of a stack (nl_stack_coverage) for gfx950: out[p] = how many of the active
// frames have a sample at p that is not NaN, i.e. the n the reference's gather leaves for the pixel
// (internal/ops/stack/stack.go:380-387; +-Inf are data).
//
// Pure streaming, the walk of stack_mean.hip: each lane owns 4 consecutive pixels (16-byte nontemporal loads, 1 KiB
// per wave instruction) and walks the frames with 8 loads in flight; one 8-byte store of four uint16 counts per
// lane.  No LDS, nothing crosses lanes.  HBM-bound: 4*N + 2 bytes per pixel.
#include "launch_common.hpp"

namespace nl {

typedef float cov_f4 __attribute__((ext_vector_type(4)));
typedef unsigned short cov_u16x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void stack_coverage_kernel(const float *frames, int64_t stride, int64_t npix,
                                                             int n_frames, uint16_t *out)
{
    const int64_t quads = npix >> 2;
    const int64_t stride4 = stride >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads;
         q += (int64_t)gridDim.x * blockDim.x) {
        const cov_f4 *fr = reinterpret_cast<const cov_f4 *>(frames) + q;
        int c[4] = {0, 0, 0, 0};
        int k = 0;
        for (; k + 8 <= n_frames; k += 8) {
            cov_f4 v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = __builtin_nontemporal_load(&fr[(int64_t)(k + u) * stride4]);
#pragma unroll
            for (int u = 0; u < 8; u++) {
                c[0] += v[u].x == v[u].x;
                c[1] += v[u].y == v[u].y;
                c[2] += v[u].z == v[u].z;
                c[3] += v[u].w == v[u].w;
            }
        }
        for (; k < n_frames; k++) {
            const cov_f4 v = __builtin_nontemporal_load(&fr[(int64_t)k * stride4]);
            c[0] += v.x == v.x;
            c[1] += v.y == v.y;
            c[2] += v.z == v.z;
            c[3] += v.w == v.w;
        }
        const cov_u16x4 r = {(unsigned short)c[0], (unsigned short)c[1], (unsigned short)c[2], (unsigned short)c[3]};
        __builtin_nontemporal_store(r, reinterpret_cast<cov_u16x4 *>(out) + q);
    }
}

// scalar variant: tail pixels, or a base pointer / stride that does not allow 16-byte loads
__global__ __launch_bounds__(256) void stack_coverage_scalar_kernel(const float *frames, int64_t stride, int64_t npix,
                                                                    int n_frames, uint16_t *out, int64_t first)
{
    for (int64_t i = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < npix;
         i += (int64_t)gridDim.x * blockDim.x) {
        int c = 0;
        for (int k = 0; k < n_frames; k++) {
            const float v = __builtin_nontemporal_load(&frames[(int64_t)k * stride + i]);
            c += v == v;
        }
        out[i] = (uint16_t)c;
    }
}

static int coverage_grid(int64_t items)
{
    int64_t g = (items + 255) / 256;
    if (g > 256 * 64) g = 256 * 64;
    if (g < 1) g = 1;
    return (int)g;
}

hipError_t launch_stack_coverage(const float *frames, int64_t stride, int64_t npix, int n_frames, uint16_t *out,
                                 hipStream_t stream)
{
    const bool vec_ok = (stride % 4 == 0) && ((reinterpret_cast<uintptr_t>(frames) & 15) == 0) &&
                        ((reinterpret_cast<uintptr_t>(out) & 7) == 0);
    Launcher L(stream);
    int64_t done = 0;
    if (vec_ok && npix >= 4) {
        const int64_t quads = npix >> 2;
        L(stack_coverage_kernel, coverage_grid(quads), 256, 0, frames, stride, npix, n_frames, out);
        if (L.err != hipSuccess) return L.err;
        done = quads << 2;
    }
    if (done < npix)
        L(stack_coverage_scalar_kernel, coverage_grid(npix - done), 256, 0, frames, stride, npix, n_frames, out, done);
    return L.err;
}

}  // namespace nl
