// deband.hip -- OpDebandHoriz / OpDebandVert (internal/ops/pre/banding.go:61-270) and NewImageBinNxN
// (internal/fits/fits.go:163-195) for gfx950, bit-exact.
//
// Stages of a deband, all on one stream:
//   deband_transpose       (vert only) the frame transposed through 64 x 64 LDS tiles into scratch, a bit copy: the
//                          columns become rows, so one select kernel serves both operators with contiguous loads
//   deband_row_percentile  one workgroup per row: the samples <= threshold are ballot-compacted as order-preserving
//                          uint32 keys (in LDS up to kDebandLdsSamples samples, else into a global staging area re-read
//                          by every pass), k = int(float32(n) * P * 0.01) is formed on the device, and the radix select
//                          of select_common.hpp gives QSelectFloat32(samples, k) as the order statistic
//                          sorted[clamp(k, 1, n) - 1].  The samples hold no NaN (NaN <= threshold is false), so the
//                          result is a function of the multiset only (up to the sign of a zero tied at that rank).
//   (host)                 one download of the percentiles and counts; the windows, fixWindowEdge (:134-162), the
//                          medians, the factors and lowest / highest literally, with bounds checks standing in for Go's
//                          panics; one upload of the factors
//   deband_scale           x * factor[row] (horiz) or x * factor[col] (vert): the one HBM-bound pass, 8 B / pixel
// The reference's panics come back as NL_ERR_INVALID_ARG with a message naming the site.
#include <math.h>

#include <algorithm>
#include <vector>

#include "deband.hpp"
#include "frame_common.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"

namespace nl {

namespace {

constexpr int kTile = 64;              // deband_transpose: 64 x 64 floats per workgroup of 256
constexpr int kScaleThreads = 256;
constexpr int kScaleCols = 4;          // columns per lane of deband_scale
constexpr int kBinThreads = 256;
constexpr size_t kLdsCap = 80 * 1024;  // LDS of one row's workgroup: two workgroups per CU (160 KiB)

struct RowPct {
    float value;                       // QSelectFloat32(samples, k); NaN when the row has no sample
    int n;                             // numSamples
};

// out[x][y] = in[y][x] for a height x width frame
__global__ __launch_bounds__(256) void deband_transpose_kernel(const float *in, int width, int height, float *out)
{
    __shared__ float tile[kTile][kTile + 1];
    const int tx = threadIdx.x & (kTile - 1), ty = threadIdx.x / kTile;
    const int x0 = blockIdx.x * kTile, y0 = blockIdx.y * kTile;
    for (int r = ty; r < kTile; r += 256 / kTile) {
        const int x = x0 + tx, y = y0 + r;
        if (x < width && y < height) tile[r][tx] = in[(int64_t)y * width + x];
    }
    __syncthreads();
    for (int r = ty; r < kTile; r += 256 / kTile) {
        const int x = x0 + r, y = y0 + tx;
        if (x < width && y < height) out[(int64_t)x * height + y] = tile[tx][r];
    }
}

// banding.go:82-93 for row blockIdx.x of rows x len.  kLds: the keys live in LDS (dynamic, after SelectShared), else
// at stage[row * len] (rows x len keys).
template <bool kLds>
__global__ __launch_bounds__(kSelectThreads) void deband_row_percentile_kernel(const float *data, int len,
                                                                               float threshold, float percentile,
                                                                               uint32_t *stage, RowPct *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    SelectShared &sh = *reinterpret_cast<SelectShared *>(lds);
    const int row = blockIdx.x;
    const float *src = data + (int64_t)row * len;
    uint32_t *keys = kLds ? reinterpret_cast<uint32_t *>(lds + ((sizeof(SelectShared) + 15) & ~(size_t)15))
                          : stage + (int64_t)row * len;
    if (threadIdx.x == 0) sh.count = 0;
    __syncthreads();

    // the samples <= threshold (:85-90); their order does not matter here
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < len; base += kSelectThreads) {
        const int i = base + threadIdx.x;
        const float v = i < len ? src[i] : 0.0f;
        const bool keep = i < len && v <= threshold;
        const unsigned long long ball = __ballot(keep);
        unsigned pos = 0;
        if (lane == 0 && ball) pos = atomicAdd(&sh.count, (unsigned)__popcll(ball));
        pos = __shfl(pos, 0, 64);
        if (keep) keys[pos + __popcll(ball & ((1ull << lane) - 1))] = f2key(v);
    }
    __syncthreads();
    const int n = (int)sh.count;
    if (n == 0) {
        if (threadIdx.x == 0) out[row] = RowPct{NAN, 0};
        return;
    }
    // k := int(float32(numSamples) * Percentile * 0.01) (:91); QSelectFloat32 takes k < 1 as 1 and k > n as n
    const float kf = (float)n * percentile * 0.01f;
    const unsigned k = kf >= 1.0f ? (unsigned)min((long long)kf, (long long)n) : 1u;
    const uint32_t key = block_select(n, k, [&](int i, uint32_t *out_key) { *out_key = keys[i]; return true; }, sh);
    if (threadIdx.x == 0) out[row] = RowPct{key2f(key), n};
}

// theRow[col] = v * factor (:123-126, :262-264).  kVec: width % 4 == 0 and a 16-byte aligned frame.
template <bool kCols, bool kVec>
__global__ __launch_bounds__(kScaleThreads) void deband_scale_kernel(float *data, int width, int col_blocks,
                                                                     const float *factor)
{
    const int y = blockIdx.x / col_blocks;
    const int x0 = ((blockIdx.x % col_blocks) * kScaleThreads + threadIdx.x) * kScaleCols;
    if (x0 >= width) return;
    float *row = data + (int64_t)y * width;
    if (kVec) {
        float4 t = *reinterpret_cast<const float4 *>(row + x0);
        float4 f;
        if (kCols) f = *reinterpret_cast<const float4 *>(factor + x0);
        else f.x = f.y = f.z = f.w = factor[y];
        t.x *= f.x; t.y *= f.y; t.z *= f.z; t.w *= f.w;
        *reinterpret_cast<float4 *>(row + x0) = t;
    } else {
        for (int u = 0; u < kScaleCols && x0 + u < width; u++) row[x0 + u] *= factor[kCols ? x0 + u : y];
    }
}

// NewImageBinNxN (fits.go:178-192): one lane per output pixel, sum over yoff then xoff from 0, then sum * normalizer.
// N: the compile-time bin size (0: n at run time).  kVec (N = 2, 4): width % N == 0 and an 8- / 16-byte aligned
// frame, every source row of the pixel is one vector load.
template <int N, bool kVec>
__global__ __launch_bounds__(kBinThreads) void bin_kernel(const float *in, int width, int n_rt, float *out, int out_w,
                                                          int out_pixels, float normalizer)
{
    const int o = blockIdx.x * kBinThreads + threadIdx.x;
    if (o >= out_pixels) return;
    const int n = N ? N : n_rt;
    const int x = o % out_w, y = o / out_w;
    const float *src = in + (int64_t)y * n * width + (int64_t)x * n;
    float sum = 0.0f;
    if (N == 2 && kVec) {
#pragma unroll
        for (int yoff = 0; yoff < 2; yoff++) {
            const float2 t = *reinterpret_cast<const float2 *>(src + (int64_t)yoff * width);
            sum += t.x; sum += t.y;
        }
    } else if (N == 4 && kVec) {
#pragma unroll
        for (int yoff = 0; yoff < 4; yoff++) {
            const float4 t = *reinterpret_cast<const float4 *>(src + (int64_t)yoff * width);
            sum += t.x; sum += t.y; sum += t.z; sum += t.w;
        }
    } else {
        for (int yoff = 0; yoff < n; yoff++)
            for (int xoff = 0; xoff < n; xoff++) sum += src[(int64_t)yoff * width + xoff];
    }
    out[o] = sum * normalizer;
}

int invalid(std::string *msg, const std::string &m)
{
    *msg = m;
    return NL_ERR_INVALID_ARG;
}

// fixWindowEdge (banding.go:134-162), literally; false where a select or an index would panic
bool fix_window_edge(std::vector<float> &window, int missing, std::vector<float> &half)
{
    const int n = (int)window.size(), n_left = n / 2, n_right = n - n_left;
    float left_median, right_median;
    half.assign(window.begin(), window.begin() + n_left);
    if (!qselect_median_lit(half.data(), n_left, &left_median)) return false;
    half.assign(window.begin() + n_left, window.end());
    if (!qselect_median_lit(half.data(), n_right, &right_median)) return false;

    const float mean_of_medians = 0.5f * (left_median + right_median);
    const float center = 0.5f * ((float)n_left + (float)n_right);
    const float slope_of_medians = (right_median - left_median) / center;

    if (missing < 0) {
        for (int i = n + missing; i < n; i++) {
            if (i < 0) return false;
            const float offset = (float)(i - n) - center;
            window[i] = mean_of_medians + slope_of_medians * offset;
        }
    } else {
        for (int i = 0; i < missing; i++) {
            if (i >= n) return false;
            const float offset = (float)(i + n) - center;
            window[i] = mean_of_medians + slope_of_medians * offset;
        }
    }
    return true;
}

}  // namespace

int deband_run(float *d_data, int width, int height, bool cols, const DebandParams &p, DebandWork &w,
               hipStream_t stream, float *lowest, float *highest, std::string *msg)
{
    const int lines = cols ? width : height;        // rows (horiz) or columns (vert) to correct
    const int len = cols ? height : width;          // samples of one of them
    const std::string op = cols ? "OpDebandVert.Apply (banding.go:197-270)" : "OpDebandHoriz.Apply (banding.go:61-132)";
    const char *line = cols ? "column" : "row";
    if (p.window <= 0)     // (vert only: horiz guards it) make([]float32, window) / QSelectMedianFloat32 of no element
        return invalid(msg, op + " panics with a window of " + std::to_string(p.window) + " columns (banding.go:207, :254)");
    const int window = std::min(p.window, lines);

    RowPct *d_pct;
    float *d_factor;
    auto carve = [&](void *base) {
        Carver c(base);
        d_pct = c.take<RowPct>(lines);
        d_factor = c.take<float>(lines);
        return align_up(c.bytes());
    };
    NL_RUN_HIP(w.buf.reserve(carve(nullptr), stream));
    carve(w.buf.ptr);

    Launcher L(stream);
    const float *src = d_data;
    if (cols) {
        NL_RUN_HIP(w.transposed.reserve(sizeof(float) * (size_t)width * height, stream));
        float *t = static_cast<float *>(w.transposed.ptr);
        L(deband_transpose_kernel, dim3((width + kTile - 1) / kTile, (height + kTile - 1) / kTile), 256, 0, d_data, width,
          height, t);
        src = t;
    }

    // the percentile of every row: LDS when the row fits the budget, else the global staging area
    int dev = 0, lds_max = 0;
    NL_RUN_HIP(hipGetDevice(&dev));
    NL_RUN_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    const size_t sh_head = (sizeof(SelectShared) + 15) & ~(size_t)15;
    const size_t lds_bytes = sh_head + sizeof(uint32_t) * (size_t)len;
    if (len <= kDebandLdsSamples && lds_bytes <= std::min(kLdsCap, (size_t)lds_max)) {
        L(deband_row_percentile_kernel<true>, lines, kSelectThreads, lds_bytes, src, len, p.threshold, p.percentile,
          nullptr, d_pct);
    } else {
        NL_RUN_HIP(w.stage.reserve(sizeof(uint32_t) * (size_t)width * height, stream));
        L(deband_row_percentile_kernel<false>, lines, kSelectThreads, sh_head, src, len, p.threshold, p.percentile,
          static_cast<uint32_t *>(w.stage.ptr), d_pct);
    }
    NL_RUN_LAUNCHED(L);
    std::vector<RowPct> got(lines);
    NL_RUN_HIP(hipMemcpyAsync(got.data(), d_pct, sizeof(RowPct) * lines, hipMemcpyDeviceToHost, stream));
    NL_RUN_HIP(hipStreamSynchronize(stream));

    std::vector<float> pct(lines);
    for (int i = 0; i < lines; i++) {
        if (got[i].n == 0)
            return invalid(msg, op + ": QSelectFloat32 (qsort.go:94-126) would index past the slice: no sample <= threshold " +
                                    std::to_string(p.threshold) + " in " + line + " " + std::to_string(i) +
                                    " (banding.go:" + (cols ? "228" : "92") + ")");
        pct[i] = got[i].value;
    }

    // the windows, their medians and the factors (:96-121, :235-259)
    std::vector<float> clone(window), half, factor(lines);
    float lo = 1.0f, hi = 0.0f;
    for (int i = 0; i < lines; i++) {
        int start = i - (window >> 1);
        int missing = 0;
        if (start < 0) {
            missing = start;
            start = 0;
        }
        int end = start + window;
        if (end > lines) {
            missing = end - lines;
            end = lines;
            start = end - window;
        }
        std::copy(pct.begin() + start, pct.begin() + end, clone.begin());
        float median;
        if ((missing != 0 && !fix_window_edge(clone, missing, half)) ||
            !qselect_median_lit(clone.data(), window, &median))
            return invalid(msg, op + ": QSelectFloat32 (qsort.go:94-126) would index past the slice selecting the median "
                                     "of the window of " + line + " " + std::to_string(i));
        const float f = median / pct[i];
        if (f < lo) lo = f;
        if (f > hi) hi = f;
        factor[i] = f;
    }

    NL_RUN_HIP(hipMemcpyAsync(d_factor, factor.data(), sizeof(float) * lines, hipMemcpyHostToDevice, stream));
    const int col_blocks = (width + kScaleThreads * kScaleCols - 1) / (kScaleThreads * kScaleCols);
    const bool vec = width % kScaleCols == 0 && ((uintptr_t)d_data & 15) == 0;
    with_bool(cols, [&](auto C) {
        with_bool(vec, [&](auto V) {
            L(deband_scale_kernel<decltype(C)::value, decltype(V)::value>, (unsigned)col_blocks * (unsigned)height,
              kScaleThreads, 0, d_data, width, col_blocks, d_factor);
        });
    });
    NL_RUN_LAUNCHED(L);
    NL_RUN_HIP(hipStreamSynchronize(stream));
    *lowest = lo;
    *highest = hi;
    return NL_OK;
}

hipError_t launch_bin(const float *d_in, int width, int height, int n, float *d_out, hipStream_t stream)
{
    const int out_w = width / n, out_h = height / n;
    const int out_pixels = out_w * out_h;
    const float normalizer = 1.0f / (float)(n * n);          // fits.go:178
    const unsigned blocks = (unsigned)((out_pixels + kBinThreads - 1) / kBinThreads);
    Launcher L(stream);
    const bool vec = width % n == 0 && ((uintptr_t)d_in & 15) == 0;
    if (n == 2 && vec)
        L(bin_kernel<2, true>, blocks, kBinThreads, 0, d_in, width, n, d_out, out_w, out_pixels, normalizer);
    else if (n == 4 && vec)
        L(bin_kernel<4, true>, blocks, kBinThreads, 0, d_in, width, n, d_out, out_w, out_pixels, normalizer);
    else
        L(bin_kernel<0, false>, blocks, kBinThreads, 0, d_in, width, n, d_out, out_w, out_pixels, normalizer);
    return L.err;
}

}  // namespace nl
