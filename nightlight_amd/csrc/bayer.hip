// bayer.hip -- the colour-camera front of preprocessing for gfx950:
//   OpBadPixel.Apply, Bayer branch   internal/ops/pre/preprocess.go:196-201: CosmeticCorrectionBayer badpixels_bayer.go:26-351
//   OpDebayer.Apply                  preprocess.go:239-251: DebayerBilinear debayer.go:41-263
//
// The correction is seven launches on one stream, no host round trip in between (BayerParams carries the
// device-computed thresholds), bit-exact including the statistics:
//   bayer_median   one lane per channel pixel: median of the same-colour neighbourhood from the ORIGINAL data, in the
//                  reference's gather order (9 values: the network; fewer, on the perimeter: QSelectMedianFloat32
//                  restated); delta = data - median and the median, compact                   (R ~9x4 B, W 8 B)
//   bayer_rowsum   per channel row, one fp32 chain left to right (deltaRowSum); 8 rows per workgroup staged through
//                  LDS, so the chains spread over every CU                                     (R 4 B)
//   bayer_total    one lane: the row totals in row order, mean = sum / float32(count)
//   bayer_rowsum<SQ>, bayer_total<SQ>   the same for (delta-mean)^2: variance, std = float32(sqrt(float64(var))),
//                  lo = -sigma_low*std, hi = sigma_high*std
//   bayer_replace  delta < lo || delta > hi: data = median (not in place: the medians are from phase 1); one workgroup
//                  per channel row, its replaced count                                          (R 8 B)
//   bayer_count    one workgroup sums the row counts (no global atomics)
// No fused multiply-add anywhere (-ffp-contract=off, as the reference's amd64 build).
// The debayer is one launch, one lane per 2x2 output box, in the reference's expression order.
#include "bayer.hpp"
#include "frame_common.hpp"
#include "launch_common.hpp"
#include "median9.hpp"

namespace nl {

namespace {

constexpr int kBayerThreads = 256;
constexpr int kSumRows = 8;          // channel rows per workgroup of bayer_rowsum
constexpr int kSumChunk = 256;       // columns staged per step
constexpr int kTotalChunk = 2048;    // row totals staged per step of bayer_total
constexpr int kCountThreads = 1024;

// sqrt2 = float32(math.Sqrt2) and the typed float32 constant 1.0/(2.0+sqrt2) of debayer.go:126-171.  go/types rounds
// a typed constant to its type after every operation: f32(1 / f32(2 + sqrt2)) = 0x1.2bec32p-2 (0.2928932), not the
// once-rounded exact value 0x1.2bec34p-2.
constexpr float kSqrt2 = 0x1.6a09e6p+0f;
constexpr float kGreenK = 0x1.2bec32p-2f;

// Workgroup i of n goes to XCD i % 8 (MI355X_MICROARCH, workgroup dispatch): hand XCD k the contiguous band
// [k*n/8, (k+1)*n/8) of logical workgroups instead, so that the raw rows a stencil shares with the rows next to it
// sit in the same L2.  A bijection on [0, n) (the tail past a multiple of 8 stays in place): speed only.
__device__ __forceinline__ unsigned xcd_band(unsigned i, unsigned n)
{
    const unsigned per = n >> 3;
    return i >= per * 8u ? i : (i & 7u) * per + (i >> 3);
}

// QSelectFloat32 (qsort.go:87-125) restated, on a private array of n <= 9 values.  The two scans stop at the ends of
// the range: with NaN-free input that never changes where they stop (the Hoare scans stop at the pivot or before);
// with a NaN pivot the reference runs off the slice and panics, here the scan stays inside.
__device__ float bayer_qselect(float *a, int n, int k)
{
    int left = 0, right = n - 1;
    while (left < right) {
        const int mid = (left + right) >> 1;
        const float pivot = a[mid];
        int l = left - 1, r = right + 1;
        for (;;) {
            do { l++; } while (l < right && !(a[l] >= pivot));
            do { r--; } while (r > left && !(a[r] <= pivot));
            if (l >= r) break;
            const float t = a[l]; a[l] = a[r]; a[r] = t;
        }
        const int offset = r - left + 1;
        if (k <= offset) {
            right = r;
        } else {
            left = r + 1;
            k -= offset;
        }
    }
    return a[left];
}

// QSelectMedianFloat32 (qsort.go:68-82): for an even count 0.5*(max of the lower part + upper)
__device__ float bayer_qselect_median(float *a, int n)
{
    const int k = (n >> 1) + 1;
    const float upper = bayer_qselect(a, n, k);
    if (n & 1) return upper;
    float lower = a[0];
    for (int i = 1; i < k - 1; i++)
        if (a[i] > lower) lower = a[i];
    return 0.5f * (lower + upper);
}

// MedianFilterBayerRedOrBlue / MedianFilterBayerGreen (badpixels_bayer.go:64-187) at one channel pixel
__device__ __forceinline__ float bayer_median_at(const float *data, const BayerGeom &g, int x, int y)
{
    const int W = g.width, H = g.height;
    const float *p = data + (int64_t)y * W + x;
    if (x >= 2 && x + 2 < W && y >= 2 && y + 2 < H) {
        if (g.green)       // gOffsets (:122-132)
            return median9_cmp(p[-2 * W], p[-W - 1], p[-W + 1], p[-2], p[0], p[2], p[W - 1], p[W + 1], p[2 * W]);
        return median9_cmp(p[-2 * W - 2], p[-2 * W], p[-2 * W + 2], p[-2], p[0], p[2], p[2 * W - 2], p[2 * W],
                           p[2 * W + 2]);
    }
    // the perimeter: neighbours outside the image are dropped, 4 - 8 values in the same order
    float a[9];
    int n = 0;
    if (g.green) {
        const int ox[9] = {0, -1, 1, -2, 0, 2, -1, 1, 0}, oy[9] = {-2, -1, -1, 0, 0, 0, 1, 1, 2};
        for (int t = 0; t < 9; t++) {
            const int nx = x + ox[t], ny = y + oy[t];
            if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            a[n++] = data[(int64_t)ny * W + nx];
        }
    } else {
        for (int dy = -2; dy <= 2; dy += 2) {
            const int ny = y + dy;
            if (ny < 0 || ny >= H) continue;
            for (int dx = -2; dx <= 2; dx += 2) {
                const int nx = x + dx;
                if (nx < 0 || nx >= W) continue;
                a[n++] = data[(int64_t)ny * W + nx];
            }
        }
    }
    return bayer_qselect_median(a, n);
}

// rows * ceil(cols / 256) workgroups, in XCD bands: lane k of a column block of channel row j
__global__ __launch_bounds__(kBayerThreads) void bayer_median_kernel(const float *data, BayerGeom g, float *delta,
                                                                      float *median)
{
    const unsigned blocks = (unsigned)(g.cols + kBayerThreads - 1) / kBayerThreads;
    const unsigned b = xcd_band(blockIdx.x, gridDim.x);
    const int j = (int)(b / blocks), k = (int)(b % blocks) * kBayerThreads + threadIdx.x;
    if (k >= bayer_row_n(g, j)) return;
    const int x = bayer_row_x(g, j) + 2 * k, y = bayer_row_y(g, j);
    const float m = bayer_median_at(data, g, x, y);
    const int64_t c = (int64_t)j * g.cstride + k;
    delta[c] = data[(int64_t)y * g.width + x] - m;
    median[c] = m;
}

// acc += s[0], s[1], ..., s[m-1] in that order (s 16-byte aligned in LDS).  The dependent adds are the price of the
// reference's order; the LDS reads of the next 16 values are issued before the adds of these 16, so the chain does
// not wait for them.
__device__ __forceinline__ float chain_add(const float *s, int m, float acc)
{
    auto ld = [&](int i) { return *reinterpret_cast<const float4 *>(s + i); };
    int i = 0;
    if (m >= 16) {
        float4 a0 = ld(0), a1 = ld(4), a2 = ld(8), a3 = ld(12);
        auto add16 = [&]() {
            acc += a0.x; acc += a0.y; acc += a0.z; acc += a0.w;
            acc += a1.x; acc += a1.y; acc += a1.z; acc += a1.w;
            acc += a2.x; acc += a2.y; acc += a2.z; acc += a2.w;
            acc += a3.x; acc += a3.y; acc += a3.z; acc += a3.w;
        };
        for (; i + 32 <= m; i += 16) {
            const float4 b0 = ld(i + 16), b1 = ld(i + 20), b2 = ld(i + 24), b3 = ld(i + 28);
            add16();
            a0 = b0; a1 = b1; a2 = b2; a3 = b3;
        }
        add16();
        i += 16;
    }
    for (; i < m; i++) acc += s[i];
    return acc;
}

// DeltaStatsBayer* (badpixels_bayer.go:190-296), one pass: per channel row a fresh fp32 accumulator summing left to
// right (delta, or (delta-mean)*(delta-mean) when SQ).  kSumRows rows per workgroup: all 256 lanes stage kSumChunk
// columns of each row through LDS (coalesced, the next chunk loaded while this one is summed), lane r < kSumRows runs
// row r's chain.
template <bool SQ>
__global__ __launch_bounds__(kBayerThreads) void bayer_rowsum_kernel(const float *delta, BayerGeom g,
                                                                      const BayerParams *p, float *rowsum)
{
    __shared__ __attribute__((aligned(16))) float tile[2][kSumRows][kSumChunk + 4];
    const int j0 = blockIdx.x * kSumRows, t = threadIdx.x;
    const float mean = SQ ? p->mean : 0.0f;
    int nrow[kSumRows];
#pragma unroll
    for (int r = 0; r < kSumRows; r++) nrow[r] = j0 + r < g.rows ? bayer_row_n(g, j0 + r) : 0;
    const int n_own = t < kSumRows && j0 + t < g.rows ? bayer_row_n(g, j0 + t) : 0;
    float v[kSumRows];
    auto load = [&](int c0) {
#pragma unroll
        for (int r = 0; r < kSumRows; r++) {
            const int c = c0 + t;
            float e = 0.0f;
            if (c < nrow[r]) {
                e = delta[(int64_t)(j0 + r) * g.cstride + c];
                if (SQ) e = (e - mean) * (e - mean);
            }
            v[r] = e;
        }
    };
    load(0);
    float acc = 0.0f;
    int buf = 0;
    for (int c0 = 0; c0 < g.cols; c0 += kSumChunk) {
#pragma unroll
        for (int r = 0; r < kSumRows; r++) tile[buf][r][t] = v[r];
        __syncthreads();
        if (c0 + kSumChunk < g.cols) load(c0 + kSumChunk);
        if (t < kSumRows) {
            const int lim = n_own - c0 < kSumChunk ? n_own - c0 : kSumChunk;
            acc = chain_add(tile[buf][t], lim, acc);
        }
        buf ^= 1;
    }
    if (t < kSumRows && j0 + t < g.rows) rowsum[j0 + t] = acc;
}

// the row totals in row order (deltaSum += deltaRowSum), one lane; then the mean, or the variance, std, thresholds
template <bool SQ>
__global__ __launch_bounds__(kBayerThreads) void bayer_total_kernel(const float *rowsum, BayerGeom g, float sigma_low,
                                                                     float sigma_high, BayerParams *p)
{
    __shared__ __attribute__((aligned(16))) float s[kTotalChunk];
    float sum = 0.0f;
    for (int j0 = 0; j0 < g.rows; j0 += kTotalChunk) {
        const int m = g.rows - j0 < kTotalChunk ? g.rows - j0 : kTotalChunk;
        float v[kTotalChunk / kBayerThreads];           // (every load in flight before the first LDS write)
#pragma unroll
        for (int q = 0; q < kTotalChunk / kBayerThreads; q++) {
            const int i = threadIdx.x + q * kBayerThreads;
            v[q] = i < m ? rowsum[j0 + i] : 0.0f;
        }
#pragma unroll
        for (int q = 0; q < kTotalChunk / kBayerThreads; q++) s[threadIdx.x + q * kBayerThreads] = v[q];
        __syncthreads();
        if (threadIdx.x == 0) sum = chain_add(s, m, sum);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float n = (float)(int)g.count;               // float32(deltaNum), deltaNum an int32
    if (!SQ) {
        p->mean = sum / n;
    } else {
        const float var = g.count > 0 ? sum / n : 0.0f;
        const float std = (float)sqrt((double)var);
        p->std = std;
        p->lo = -sigma_low * std;
        p->hi = sigma_high * std;
    }
}

// ReplaceOutliersBayer* (badpixels_bayer.go:299-351); one workgroup per channel row, its count to removed[row]
__global__ __launch_bounds__(kBayerThreads) void bayer_replace_kernel(float *data, const float *delta,
                                                                       const float *median, BayerGeom g,
                                                                       const BayerParams *p, unsigned *removed)
{
    __shared__ unsigned s_wave[kBayerThreads / 64];
    const int j = blockIdx.x, n = bayer_row_n(g, j);
    const float lo = p->lo, hi = p->hi;
    float *row = data + (int64_t)bayer_row_y(g, j) * g.width + bayer_row_x(g, j);
    unsigned count = 0;
    for (int k = threadIdx.x; k < n; k += kBayerThreads) {
        const int64_t c = (int64_t)j * g.cstride + k;
        const float d = delta[c];
        if (d < lo || d > hi) {
            row[2 * k] = median[c];
            count++;
        }
    }
    wave_values(wave_sum(count), s_wave);
    if (threadIdx.x == 0) removed[j] = sum_in_order<kBayerThreads / 64>(s_wave);
}

__global__ __launch_bounds__(kCountThreads) void bayer_count_kernel(const unsigned *removed, int64_t blocks,
                                                                     BayerParams *p)
{
    __shared__ unsigned long long s_wave[kCountThreads / 64];
    unsigned long long sum = 0;
    for (int64_t b = threadIdx.x; b < blocks; b += kCountThreads) sum += removed[b];
    wave_values(wave_sum(sum), s_wave);
    if (threadIdx.x == 0) p->removed = sum_in_order<kCountThreads / 64>(s_wave);
}

// DebayerBilinearRGGBTo{Red,Green,Blue} (debayer.go:63-263), one lane per 2x2 box of the output; box rows * blocks
// of 256 boxes per row workgroups, in XCD bands.  Sums left to right
// as written; V2: the two values of an output row as one 8-byte store (out and out_stride even-aligned).
template <int CH, bool V2>
__global__ __launch_bounds__(kBayerThreads) void debayer_kernel(const float *data, int width, int height, int xo,
                                                                 int yo, int adj_w, float *out, int64_t out_stride)
{
    const unsigned blocks = (unsigned)((adj_w >> 1) + kBayerThreads - 1) / kBayerThreads;
    const unsigned b = xcd_band(blockIdx.x, gridDim.x);
    const int bx = (int)(b % blocks) * kBayerThreads + threadIdx.x;
    if (bx >= (adj_w >> 1)) return;
    const int row = 2 * (int)(b / blocks), col = 2 * bx;
    const int64_t W = width;
    const float *src = data + (int64_t)(row + yo) * W + (col + xo);
    const bool has_left = col + xo > 0, has_up = row + yo > 0;
    const bool has_right = col + xo < width - 2, has_down = row + yo < height - 2;
    float o0, o1, o2, o3;
    if (CH == kBayerR) {                                          // :87-111
        const float r = src[0];
        float r_right = r, r_down = r, r_rd = r;
        if (has_right) {
            r_right = src[2];
            if (has_down) {
                r_down = src[2 * W];
                r_rd = src[2 + 2 * W];
            }
        } else if (has_down) {
            r_down = src[2 * W];
        }
        o0 = r;
        o1 = 0.5f * (r + r_right);
        o2 = 0.5f * (r + r_down);
        o3 = 0.25f * (r + r_right + r_down + r_rd);
    } else if (CH == kBayerG) {                                   // :152-186
        const float g1 = src[1], g2 = src[W];
        const float fb1 = (2.0f * g1 + kSqrt2 * g2) * kGreenK;    // the edge fallbacks
        const float fb2 = (kSqrt2 * g1 + 2.0f * g2) * kGreenK;
        const float g1_left = has_left ? src[-1] : fb1;
        const float g2_up = has_up ? src[-W] : fb2;
        const float g2_right = has_right ? src[2 + W] : fb1;
        const float g1_down = has_down ? src[1 + 2 * W] : fb2;
        o0 = 0.25f * (g1 + g2 + g1_left + g2_up);
        o1 = g1;
        o2 = g2;
        o3 = 0.25f * (g1 + g2 + g2_right + g1_down);
    } else {                                                      // :225-249
        const float b = src[1 + W];
        float b_left = b, b_up = b, b_lu = b;
        if (has_left) {
            b_left = src[-1 + W];
            if (has_up) {
                b_up = src[1 - W];
                b_lu = src[-1 - W];
            }
        } else if (has_up) {
            b_up = src[1 - W];
        }
        o0 = 0.25f * (b + b_left + b_up + b_lu);
        o1 = 0.5f * (b + b_up);
        o2 = 0.5f * (b + b_left);
        o3 = b;
    }
    float *d = out + (int64_t)row * out_stride + col;
    if (V2) {
        *reinterpret_cast<float2 *>(d) = float2{o0, o1};
        *reinterpret_cast<float2 *>(d + out_stride) = float2{o2, o3};
    } else {
        d[0] = o0;
        d[1] = o1;
        d[out_stride] = o2;
        d[out_stride + 1] = o3;
    }
}

}  // namespace

BayerGeom bayer_geom(int width, int height, int channel, int xo, int yo)
{
    BayerGeom g;
    g.width = width;
    g.height = height;
    g.green = channel == kBayerG;
    g.x0 = channel == kBayerB ? xo + 1 : xo;
    g.y0 = channel == kBayerB ? yo + 1 : yo;
    if (g.green) g.rows = g.y0 < height ? height - g.y0 : 0;
    else g.rows = g.y0 < height ? (height - g.y0 + 1) >> 1 : 0;
    g.cols = 0;
    g.count = 0;
    for (int j = 0; j < 2 && j < g.rows; j++) {              // (rows alternate between two lengths at most)
        const int n = bayer_row_n(g, j);
        if (n > g.cols) g.cols = n;
        const int64_t like_j = g.green ? (j == 0 ? (g.rows + 1) >> 1 : g.rows >> 1) : g.rows;
        g.count += like_j * n;
        if (!g.green) break;
    }
    g.cstride = (g.cols + 63) & ~63;
    return g;
}

int64_t bayer_replace_blocks(const BayerGeom &g) { return g.rows; }

hipError_t launch_bayer_correct(float *data, const BayerGeom &g, float sigma_low, float sigma_high,
                                const BayerScratch &s, hipStream_t stream)
{
    const unsigned grid = (unsigned)(g.rows * ((g.cols + kBayerThreads - 1) / kBayerThreads));
    const bool any = g.rows > 0 && g.cols > 0;         // (a row without a channel pixel still sums to +0)
    const unsigned sum_blocks = (unsigned)((g.rows + kSumRows - 1) / kSumRows);
    Launcher L(stream);
    if (any) L(bayer_median_kernel, grid, kBayerThreads, 0, data, g, s.delta, s.median);
    if (g.rows > 0) L(bayer_rowsum_kernel<false>, sum_blocks, kBayerThreads, 0, s.delta, g, s.params, s.rowsum);
    L(bayer_total_kernel<false>, 1, kBayerThreads, 0, s.rowsum, g, sigma_low, sigma_high, s.params);
    if (g.rows > 0) L(bayer_rowsum_kernel<true>, sum_blocks, kBayerThreads, 0, s.delta, g, s.params, s.rowsum);
    L(bayer_total_kernel<true>, 1, kBayerThreads, 0, s.rowsum, g, sigma_low, sigma_high, s.params);
    if (any) L(bayer_replace_kernel, (unsigned)g.rows, kBayerThreads, 0, data, s.delta, s.median, g, s.params, s.removed);
    L(bayer_count_kernel, 1, kCountThreads, 0, s.removed, any ? bayer_replace_blocks(g) : (int64_t)0, s.params);
    return L.err;
}

hipError_t launch_debayer(const float *data, int width, int height, int channel, int xo, int yo, float *out,
                          int64_t out_stride, hipStream_t stream)
{
    const int adj_w = (width - xo) & ~1, adj_h = (height - yo) & ~1;
    if (adj_w <= 0 || adj_h <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((adj_h >> 1) * (((adj_w >> 1) + kBayerThreads - 1) / kBayerThreads));
    const bool v2 = ((uintptr_t)out & 7) == 0 && (out_stride & 1) == 0;
    Launcher L(stream);
    with_class<kBayerR, kBayerG, kBayerB>(channel, [&](auto CH) {          // (channel is one of the three)
        with_bool(v2, [&](auto V2) {
            L(debayer_kernel<decltype(CH)::value, decltype(V2)::value>, grid, kBayerThreads, 0, data, width, height, xo,
              yo, adj_w, out, out_stride);
        });
    });
    return L.err;
}

}  // namespace nl
