// blur.hip -- GaussianBlur / UnsharpMask (internal/ops/stretch/usm.go) for gfx950, bit-exact given the taps.
//
// The reference's two passes, both on one stream:
//   blur_row_kernel        Convolve1DX (usm.go:85-98) from the frame into the handle's scratch frame
//   blur_col_kernel<kUsm>  Convolve1DY (usm.go:101-114) from the scratch frame back into the frame; kUsm: with
//                          ApplyUnsharpMask (usm.go:134-149) as its epilogue, which reads the frame at the pixel it
//                          writes and nowhere else -- so both operators run in place with one scratch frame
// Every output is sum = 0.0f, then sum = sum + data[reflect(. + i)] * tap[i + k] for i = -k .. k, one fp32 multiply and
// one fp32 add each (the library is built with -ffp-contract=off), nothing reassociated, the taps' symmetry unused.
// A lane owns four columns of one row in both passes, so a wave reads and writes whole contiguous row segments.
// kStaged: the workgroup first stages its source tile and the reflected halo in LDS and every tap is an LDS read; else
// (a radius beyond kBlurRowStagedRadius / kBlurColStagedRadius) every tap is a global load.  kVec (width % 4 == 0 and
// 16-byte aligned frames): 16-byte global loads and stores, else dword ones.
#include <math.h>

#include "blur.hpp"
#include "launch_common.hpp"

namespace nl {

namespace {

constexpr int kThreads = 256;
constexpr int kTileW = 256;                                     // columns of a tile: 64 lanes x 4
constexpr int kRowTileH = 16;                                   // rows of a row-pass tile: 4 waves x 4 rows
constexpr int kRowPitch = kTileW + 2 * kBlurRowStagedRadius + 4;   // tile columns, both halos, one spare 16-byte group
constexpr int kColLdsRows = 64;                                 // rows of a column-pass tile, both halos included
static_assert(kBlurRowStagedRadius % 4 == 0 && kRowPitch % 4 == 0, "16-byte groups of a staged row");
static_assert(kColLdsRows - 2 * kBlurColStagedRadius >= 16, "output rows of a column tile");

// usm.go:25-33; in range for -size <= x < 2 * size
__device__ __forceinline__ int reflect(int size, int x)
{
    if (x < 0) return -x - 1;
    if (x >= size) return 2 * size - x - 1;
    return x;
}

// Convolve1DX for the tile of columns [x0, x0 + kTileW) and rows [y0, y0 + kRowTileH), workgroup blockIdx.x of
// col_blocks per tile row.
// kStaged: every wave stages its four rows, columns x0 - halo .. x0 + kTileW + halo - 1 (halo = the radius rounded up
// to 4, so the tile's own columns sit on 16-byte groups) at tile column c = column - x0 + halo; lane l then owns
// columns x0 + 4 l .. 4 l + 3 and walks the row's window 4 l .. in 16-byte LDS reads, tap t of output u at window
// float u + (halo - k) + t: the taps are visited in "virtual" positions o .. o + n_taps - 1 so that every register
// index is a constant.  !kVec: the four sums go back through the (dead) row in LDS so that lane l stores columns
// 64 u + l.
// !kStaged: lane l owns columns x0 + 64 u + l and loads every tap from global memory.
template <bool kStaged, bool kVec>
__global__ __launch_bounds__(kThreads) void blur_row_kernel(const float *src, int width, int height, int col_blocks,
                                                            const float *__restrict__ taps, int n_taps, float *dst)
{
    const int k = n_taps >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int x0 = (blockIdx.x % col_blocks) * kTileW, y0 = (blockIdx.x / col_blocks) * kRowTileH;
    if constexpr (kStaged) {
        __shared__ __attribute__((aligned(16))) float tile[kRowTileH * kRowPitch];
        const int halo = (k + 3) & ~3;
        const int cols = min(kTileW, width - x0);                 // (kVec: a multiple of 4)
#pragma unroll 1
        for (int q = 0; q < kRowTileH / 4; q++) {
            const int r = wave * (kRowTileH / 4) + q, y = y0 + r;
            if (y >= height) break;
            const float *srow = src + (int64_t)y * width;
            float *trow = tile + r * kRowPitch;
            if (kVec && 4 * lane < cols)
                *reinterpret_cast<float4 *>(trow + halo + 4 * lane) = *reinterpret_cast<const float4 *>(srow + x0 + 4 * lane);
            // the halos, and everything where no 16-byte group applies: one reflected dword each
            auto edge = [&](int c) {
                const int s = x0 - halo + c;
                if (s >= -k && s < width + k) trow[c] = srow[reflect(width, s)];
            };
            for (int c = lane; c < halo; c += 64) edge(c);
            for (int c = halo + (kVec ? cols : 0) + lane; c < 2 * halo + kTileW; c += 64) edge(c);
        }
        __syncthreads();
        const int o = halo - k, end = o + n_taps;
#pragma unroll 1
        for (int q = 0; q < kRowTileH / 4; q++) {
            const int r = wave * (kRowTileH / 4) + q, y = y0 + r;
            const bool live = y < height;                         // (one value per wave)
            float *trow = tile + r * kRowPitch;
            float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (live) {
                const float4 *win = reinterpret_cast<const float4 *>(trow + 4 * lane);
                float4 cur = win[0];
                for (int j = 0; 4 * j < end; j++) {
                    const float4 nxt = win[j + 1];
                    const float w[7] = {cur.x, cur.y, cur.z, cur.w, nxt.x, nxt.y, nxt.z};
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        const int t = 4 * j + v - o;
                        if (t >= 0 && t < n_taps) {
                            const float tap = taps[t];
#pragma unroll
                            for (int u = 0; u < 4; u++) sum[u] = sum[u] + w[u + v] * tap;
                        }
                    }
                    cur = nxt;
                }
            }
            const int64_t at = (int64_t)y * width + x0;
            if (kVec) {
                if (live && 4 * lane < cols) *reinterpret_cast<float4 *>(dst + at + 4 * lane) = make_float4(sum[0], sum[1], sum[2], sum[3]);
            } else {
                __syncthreads();
                if (live) *reinterpret_cast<float4 *>(trow + 4 * lane) = make_float4(sum[0], sum[1], sum[2], sum[3]);
                __syncthreads();
                if (live) {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (64 * u + lane < cols) dst[at + 64 * u + lane] = trow[64 * u + lane];
                }
            }
        }
    } else {
        const int y = y0 + threadIdx.x / 64 * (kRowTileH / 4);
#pragma unroll 1
        for (int q = 0; q < kRowTileH / 4 && y + q < height; q++) {
            const float *srow = src + (int64_t)(y + q) * width;
            float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int t = 0; t < n_taps; t++) {
                const float tap = taps[t];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int x = x0 + 64 * u + lane;
                    if (x < width) sum[u] = sum[u] + srow[reflect(width, x + t - k)] * tap;
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (x0 + 64 * u + lane < width) dst[(int64_t)(y + q) * width + x0 + 64 * u + lane] = sum[u];
        }
    }
}

// ApplyUnsharpMask (usm.go:136-147) for one pixel: d < absThreshold copies d (a NaN d or threshold fails the test and
// is sharpened), r < min before r > max
__device__ __forceinline__ float unsharp(float d, float blurred, const UsmParams &p)
{
    if (d < p.abs_threshold) return d;
    float r = d + (d - blurred) * p.gain;
    if (r < p.min) r = p.min;
    if (r > p.max) r = p.max;
    return r;
}

// Convolve1DY for the tile of columns [x0, x0 + kTileW) and out_rows = kColLdsRows - 2 k rows from y0 (kStaged) or
// kRowTileH rows (!kStaged), workgroup blockIdx.x of col_blocks per tile row; lane l owns columns x0 + 4 l + u (kVec)
// or x0 + 64 u + l.  kStaged: tile row r holds row reflect(y0 - k + r) of tmp, staged once; tap t of output row ly is
// tile row ly + t.  kUsm: dst[i] = unsharp(src[i], sum, p) -- src may be dst.
template <bool kStaged, bool kVec, bool kUsm>
__global__ __launch_bounds__(kThreads) void blur_col_kernel(const float *tmp, int width, int height, int col_blocks,
                                                            const float *__restrict__ taps, int n_taps,
                                                            const float *src, float *dst, UsmParams p)
{
    const int k = n_taps >> 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int out_rows = kStaged ? kColLdsRows - 2 * k : kRowTileH;
    const int x0 = (blockIdx.x % col_blocks) * kTileW, y0 = (blockIdx.x / col_blocks) * out_rows;
    const int rows_here = min(out_rows, height - y0);
    int col[4];
    bool in[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        col[u] = kVec ? 4 * lane + u : 64 * u + lane;
        in[u] = x0 + col[u] < width;
    }
    __shared__ __attribute__((aligned(16))) float tile[kStaged ? kColLdsRows * kTileW : 4];
    if constexpr (kStaged) {
        for (int r = wave; r < rows_here + 2 * k; r += kThreads / 64) {
            const float *srow = tmp + (int64_t)reflect(height, y0 - k + r) * width + x0;
            float *trow = tile + r * kTileW;
            if (kVec) {
                if (in[0]) *reinterpret_cast<float4 *>(trow + 4 * lane) = *reinterpret_cast<const float4 *>(srow + 4 * lane);
            } else {
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (in[u]) trow[col[u]] = srow[col[u]];
            }
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int ly = wave; ly < rows_here; ly += kThreads / 64) {
        const int y = y0 + ly;
        float sum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int t = 0; t < n_taps; t++) {
            const float tap = taps[t];
            float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (kStaged) {
                const float *trow = tile + (ly + t) * kTileW;
                if (kVec) {
                    const float4 q = *reinterpret_cast<const float4 *>(trow + 4 * lane);
                    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
                } else {
#pragma unroll
                    for (int u = 0; u < 4; u++) v[u] = trow[col[u]];
                }
            } else {
                const float *srow = tmp + (int64_t)reflect(height, y + t - k) * width + x0;
#pragma unroll
                for (int u = 0; u < 4; u++)
                    if (in[u]) v[u] = srow[col[u]];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) sum[u] = sum[u] + v[u] * tap;
        }
        const int64_t at = (int64_t)y * width + x0;
        if (kVec) {
            if (in[0]) {
                float4 out = make_float4(sum[0], sum[1], sum[2], sum[3]);
                if (kUsm) {
                    const float4 d = *reinterpret_cast<const float4 *>(src + at + 4 * lane);
                    out = make_float4(unsharp(d.x, out.x, p), unsharp(d.y, out.y, p), unsharp(d.z, out.z, p),
                                      unsharp(d.w, out.w, p));
                }
                *reinterpret_cast<float4 *>(dst + at + 4 * lane) = out;
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (in[u]) dst[at + col[u]] = kUsm ? unsharp(src[at + col[u]], sum[u], p) : sum[u];
        }
    }
}

int invalid(std::string *msg, const std::string &m)
{
    *msg = m;
    return NL_ERR_INVALID_ARG;
}

// GaussianDefiniteIntegral (usm.go:36-38) with mu = 0 (x - 0 is x): fp32 but for the erf
float gaussian_definite_integral(float sigma, float x)
{
    const float sqrt2 = (float)M_SQRT2;
    const float arg = x / (sqrt2 * sigma);
    return 0.5f * (1.0f + (float)erf((double)arg));
}

}  // namespace

int gaussian_kernel_1d(float sigma, std::vector<float> &taps, std::string *msg)
{
    const std::string site = "GaussianKernel1D (usm.go:41-82)";
    if (!(sigma > 0.0f) || sigma == INFINITY)      // NaN, negative, +Inf: the radius search never ends; 0: 0 / 0
        return invalid(msg, site + " cannot take sigma " + std::to_string(sigma) + ": its radius search (usm.go:47-54) does not end");
    const float accept_out = 0.01f;
    int radius = 0;
    for (;;) {
        const float val = gaussian_definite_integral(sigma, -0.5f - (float)radius);
        if (val < accept_out) {
            radius--;
            break;
        }
        radius++;
        if (radius > kBlurMaxRadius)
            return invalid(msg, site + ": sigma " + std::to_string(sigma) + " needs a radius above " +
                                    std::to_string(kBlurMaxRadius) + " (usm.go:47-54)");
    }
    if (radius < 0)
        return invalid(msg, site + " panics for sigma " + std::to_string(sigma) + ": radius -1, make with a negative length (usm.go:55-56)");
    taps.assign((size_t)(2 * radius + 1), 0.0f);

    float sum = 0.0f;
    float lower = gaussian_definite_integral(sigma, -0.5f - (float)radius);
    for (int i = 0; i <= radius; i++) {
        const float upper = gaussian_definite_integral(sigma, -0.5f - (float)radius + (float)(i + 1));
        const float delta = upper - lower;
        taps[i] = delta;
        sum += delta;
        lower = upper;
    }
    for (int i = 1; i <= radius; i++) {
        const float value = taps[radius - i];
        taps[radius + i] = value;
        sum += value;
    }
    const float factor = 1.0f / sum;
    for (float &t : taps) t *= factor;
    return NL_OK;
}

int blur_run(float *d_data, int width, int height, const float *taps, int n_taps, const UsmParams *usm, BlurWork &w,
             hipStream_t stream, std::string *msg)
{
    const int k = n_taps / 2;
    if (k > width || k > height)
        return invalid(msg, "Convolve1DX / Convolve1DY (usm.go:85-114): a radius of " + std::to_string(k) + " on a " +
                                std::to_string(width) + "x" + std::to_string(height) +
                                " frame: one reflect (usm.go:25-33) leaves the range");
    NL_RUN_HIP(w.tmp.reserve(sizeof(float) * (size_t)width * height, stream));
    NL_RUN_HIP(w.taps.reserve(sizeof(float) * (size_t)n_taps, stream));
    float *d_tmp = static_cast<float *>(w.tmp.ptr);
    const float *d_taps = static_cast<const float *>(w.taps.ptr);
    NL_RUN_HIP(hipMemcpyAsync(w.taps.ptr, taps, sizeof(float) * (size_t)n_taps, hipMemcpyHostToDevice, stream));

    const int col_blocks = (width + kTileW - 1) / kTileW;
    const bool vec = width % 4 == 0 && (((uintptr_t)d_data | (uintptr_t)d_tmp) & 15) == 0;
    const bool row_staged = k <= kBlurRowStagedRadius, col_staged = k <= kBlurColStagedRadius;
    const int col_rows = col_staged ? kColLdsRows - 2 * k : kRowTileH;
    const unsigned row_grid = (unsigned)col_blocks * (unsigned)((height + kRowTileH - 1) / kRowTileH);
    const unsigned col_grid = (unsigned)col_blocks * (unsigned)((height + col_rows - 1) / col_rows);
    const UsmParams p = usm ? *usm : UsmParams{0.0f, 0.0f, 0.0f, 0.0f};
    Launcher L(stream);
    if (!row_staged)
        L(blur_row_kernel<false, false>, row_grid, kThreads, 0, d_data, width, height, col_blocks, d_taps, n_taps, d_tmp);
    else
        with_bool(vec, [&](auto V) {
            L(blur_row_kernel<true, decltype(V)::value>, row_grid, kThreads, 0, d_data, width, height, col_blocks, d_taps,
              n_taps, d_tmp);
        });
    with_bool(usm != nullptr, [&](auto U) {
        if (!col_staged)
            L(blur_col_kernel<false, false, decltype(U)::value>, col_grid, kThreads, 0, d_tmp, width, height, col_blocks,
              d_taps, n_taps, d_data, d_data, p);
        else
            with_bool(vec, [&](auto V) {
                L(blur_col_kernel<true, decltype(V)::value, decltype(U)::value>, col_grid, kThreads, 0, d_tmp, width,
                  height, col_blocks, d_taps, n_taps, d_data, d_data, p);
            });
    });
    NL_RUN_LAUNCHED(L);
    NL_RUN_HIP(hipStreamSynchronize(stream));          // (the caller's taps must not be retained)
    return NL_OK;
}

}  // namespace nl
