// preprocess.hip -- the per-frame steps in front of the stack for gfx950 (mono forms):
//   OpCalibrate.Apply   internal/ops/pre/preprocess.go:68-99, Subtract / Divide badpixels.go:107-123
//   OpBadPixel.Apply    preprocess.go:180-195: BadPixelMap badpixels.go:32-51, MedianFilterSparse :81-88
//
// Calibrate is one elementwise stream.  The bad-pixel step is eight launches on one stream, no host
// round trip in between (BpParams carries the device-computed thresholds from launch to launch):
//   bp_diff        diff = data - median3x3(data), border diff = x - x; fp64 partial sums       (R 4 B, W 4 B)
//   bp_mean        one workgroup: mean = float32(sum / n)                                     (stats.go:264-277)
//   bp_variance    fp64 sum of (double)(diff - mean)^2                                         (R 4 B)
//   bp_threshold   one workgroup: std = float32(sqrt(var / n)), lo = -std*sl, hi = std*sh     (stats.go:134-144)
//   bp_classify    bad = diff < lo || diff > hi.  A bad pixel none of whose four EARLIER neighbours (i-W-1, i-W,
//                  i-W+1, i-1) is bad is replaced here, in place and in parallel; the others ("chained") go to a
//                  per-workgroup list in index order                                           (R 4 B)
//   bp_scan, bp_gather   the per-workgroup lists -> one list in index order, the bad-pixel count
//   bp_walk        one workgroup replaces the chained pixels in rounds of pairwise non-adjacent rows
// Why this equals the sequential walk of MedianFilterSparse, in short: the
// sequential walk gives every bad pixel its earlier neighbours' FINAL values and its later neighbours' ORIGINAL
// ones.  An unchained bad pixel has no bad earlier neighbour, and all its bad later neighbours are chained (it is
// their bad earlier neighbour), so before any chained pixel is written it reads exactly what the walk gives it; two
// unchained pixels are never neighbours, so their writes do not race.  The chained pixels are then walked in
// rounds: a chained pixel's earlier neighbours lie in the row above (final once an earlier round wrote them) or to
// its left in the same run of chained pixels, which one lane walks left to right.
#include "frame_common.hpp"
#include "launch_common.hpp"
#include "median9.hpp"
#include "preprocess.hpp"

namespace nl {

namespace {

constexpr int kBpThreads = 256;
constexpr int kWalkThreads = 1024;
constexpr int kScanThreads = 1024;

__device__ __forceinline__ float calib_one(float x, float d, float f, float flat_max, bool dark, bool flat)
{
    if (dark) x = x - d;                                 // Subtract, badpixels.go:107-111
    if (flat && !(f <= 0.0f)) x = x * flat_max / f;      // Divide, badpixels.go:114-123: (a*bMax)/b, b <= 0 keeps a
    return x;
}

template <bool DARK, bool FLAT, bool VEC>
__global__ __launch_bounds__(256) void calibrate_kernel(const float *in, float *out, int64_t n, const float *dark,
                                                         const float *flat, float flat_max)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (VEC) {
        const int64_t quads = n >> 2;
        for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += stride) {
            const float4 v = reinterpret_cast<const float4 *>(in)[q];
            const float4 d = DARK ? reinterpret_cast<const float4 *>(dark)[q] : float4{};
            const float4 f = FLAT ? reinterpret_cast<const float4 *>(flat)[q] : float4{};
            float4 r;
            r.x = calib_one(v.x, d.x, f.x, flat_max, DARK, FLAT);
            r.y = calib_one(v.y, d.y, f.y, flat_max, DARK, FLAT);
            r.z = calib_one(v.z, d.z, f.z, flat_max, DARK, FLAT);
            r.w = calib_one(v.w, d.w, f.w, flat_max, DARK, FLAT);
            reinterpret_cast<float4 *>(out)[q] = r;
        }
        if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
            const int64_t i = (quads << 2) + threadIdx.x;
            out[i] = calib_one(in[i], DARK ? dark[i] : 0.0f, FLAT ? flat[i] : 0.0f, flat_max, DARK, FLAT);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
            out[i] = calib_one(in[i], DARK ? dark[i] : 0.0f, FLAT ? flat[i] : 0.0f, flat_max, DARK, FLAT);
    }
}

// diff = data - MedianFilter3x3(data) (badpixels.go:34-35); the filter copies the border, so the border's diff is
// x - x (0, or NaN for a non-finite x, which then makes the std NaN as in the reference).  Rows over workgroups,
// columns over lanes: no per-pixel division.
__global__ __launch_bounds__(kBpThreads) void bp_diff_kernel(const float *data, float *diff, int width, int height,
                                                              double *partial)
{
    double sum = 0.0;
    for (int y = blockIdx.x; y < height; y += gridDim.x) {
        const float *r1 = data + (int64_t)y * width;
        const bool edge_row = y == 0 || y == height - 1;
        for (int x = threadIdx.x; x < width; x += kBpThreads) {
            const float v = r1[x];
            float med = v;
            if (!edge_row && x != 0 && x != width - 1) {
                const float *r0 = r1 - width, *r2 = r1 + width;
                med = median9(r0[x - 1], r0[x], r0[x + 1], r1[x - 1], v, r1[x + 1], r2[x - 1], r2[x], r2[x + 1]);
            }
            const float d = v - med;
            diff[(int64_t)y * width + x] = d;
            sum += (double)d;
        }
    }
    sum = block_sum<kBpThreads>(sum);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// Stats.Mean (stats.go:264-277): float32(sum / n), the sum in fp64
__global__ __launch_bounds__(kBpThreads) void bp_mean_kernel(const double *partial, int blocks, int64_t n,
                                                              BpParams *p)
{
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kBpThreads) s += partial[b];
    s = block_sum<kBpThreads>(s);
    if (threadIdx.x == 0) {
        p->mean = (float)(s / (double)n);
    }
}

// calcVariance (stats.go:280-287) around the device mean
__global__ __launch_bounds__(kBpThreads) void bp_variance_kernel(const float *diff, int64_t n, const BpParams *p,
                                                                  double *partial)
{
    const float mean = p->mean;
    double sum = 0.0;
    const int64_t quads = n >> 2;
    const float4 *d4 = reinterpret_cast<const float4 *>(diff);
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = d4[q];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const double d = (double)(e[j] - mean);
            sum += d * d;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const double d = (double)(diff[(quads << 2) + threadIdx.x] - mean);
        sum += d * d;
    }
    sum = block_sum<kBpThreads>(sum);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// StdDev (stats.go:134-144) and the thresholds of BadPixelMap (badpixels.go:38-39), fp32 as there
__global__ __launch_bounds__(kBpThreads) void bp_threshold_kernel(const double *partial, int blocks, int64_t n,
                                                                   float sigma_low, float sigma_high, BpParams *p)
{
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kBpThreads) s += partial[b];
    s = block_sum<kBpThreads>(s);
    if (threadIdx.x == 0) {
        const float std = (float)sqrt(s / (double)n);
        p->std = std;
        p->lo = -std * sigma_low;
        p->hi = std * sigma_high;
    }
}

// bad(i) for a pixel whose 3x3 neighbourhood lies inside the image.  The border's diff is 0 or NaN, never outside
// thresholds of non-negative sigmas: the interior test only keeps every read below in bounds.
__device__ __forceinline__ bool bp_bad(const float *diff, int64_t i, int width, int height, float lo, float hi)
{
    const int64_t y = i / width, x = i - y * width;
    if (y == 0 || y == height - 1 || x == 0 || x == width - 1) return false;
    const float d = diff[i];
    return d < lo || d > hi;
}

__device__ __forceinline__ float bp_median_at(const float *data, int64_t i, int width)
{
    const float *r0 = data + i - width, *r1 = data + i, *r2 = data + i + width;
    return median9(r0[-1], r0[0], r0[1], r1[-1], r1[0], r1[1], r2[-1], r2[0], r2[1]);
}

// One workgroup per kBpChunk pixels, 256 consecutive pixels per step.  Unchained bad pixels are replaced at once;
// chained ones are appended to seg[block * kBpChunk ...] in index order (wave ballot ranks + the four wave counts),
// their number to count[block], the number of bad pixels to removed[block] (summed by bp_scan: no atomics -- one
// atomic per wave on one address serialised to 290 us per 4096^2 frame).
__global__ __launch_bounds__(kBpThreads) void bp_classify_kernel(float *data, const float *diff, int width, int height,
                                                                  const BpParams *p, unsigned *seg, unsigned *count,
                                                                  unsigned *removed_count)
{
    __shared__ unsigned s_wave[kBpThreads / 64], s_bad[kBpThreads / 64];
    const float lo = p->lo, hi = p->hi;
    const int64_t n = (int64_t)width * height;
    const int64_t base = (int64_t)blockIdx.x * kBpChunk;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned removed = 0, listed = 0;
    for (int step = 0; step < kBpChunk / kBpThreads; step++) {
        const int64_t i = base + step * kBpThreads + threadIdx.x;
        bool bad = false, chained = false;
        if (i < n) {
            const float d = diff[i];
            if (d < lo || d > hi) {
                bad = bp_bad(diff, i, width, height, lo, hi);
                if (bad)
                    chained = bp_bad(diff, i - width - 1, width, height, lo, hi) ||
                              bp_bad(diff, i - width, width, height, lo, hi) ||
                              bp_bad(diff, i - width + 1, width, height, lo, hi) ||
                              bp_bad(diff, i - 1, width, height, lo, hi);
            }
        }
        if (bad && !chained) data[i] = bp_median_at(data, i, width);
        const unsigned long long bad_mask = __ballot(bad);
        const unsigned long long ch_mask = __ballot(chained);
        if (lane == 0) {
            s_wave[wave] = (unsigned)__popcll(ch_mask);
            s_bad[wave] = (unsigned)__popcll(bad_mask);
        }
        __syncthreads();
        unsigned before = listed;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        unsigned total = 0;
        for (int w = 0; w < kBpThreads / 64; w++) {
            total += s_wave[w];
            removed += s_bad[w];
        }
        if (chained) seg[base + before + lane_rank(ch_mask, lane)] = (unsigned)i;
        listed += total;
        __syncthreads();                                   // s_wave / s_bad are rewritten by the next step
    }
    if (threadIdx.x == 0) {
        count[blockIdx.x] = listed;
        removed_count[blockIdx.x] = removed;
    }
}

// Exclusive scan of the per-workgroup list lengths (one workgroup; lengths are at most kBpChunk)
__global__ __launch_bounds__(kScanThreads) void bp_scan_kernel(const unsigned *count, const unsigned *removed_count,
                                                                unsigned *offset, int blocks, BpParams *p)
{
    __shared__ unsigned s_wave[kScanThreads / 64];
    __shared__ unsigned long long s_removed;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_removed = 0;
    unsigned carry = 0;
    unsigned long long removed = 0;
    for (int b0 = 0; b0 < blocks; b0 += kScanThreads) {
        const int b = b0 + threadIdx.x;
        const unsigned v = b < blocks ? count[b] : 0u;
        removed += b < blocks ? removed_count[b] : 0u;
        unsigned incl = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned t = __shfl_up(incl, off, 64);
            if (lane >= off) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        unsigned before = carry;
        for (int w = 0; w < wave; w++) before += s_wave[w];
        unsigned total = 0;
        for (int w = 0; w < kScanThreads / 64; w++) total += s_wave[w];
        if (b < blocks) offset[b] = before + incl - v;
        carry += total;
        __syncthreads();
    }
    removed = wave_sum(removed);
    if (lane == 0) atomicAdd(&s_removed, removed);        // (LDS, 16 waves)
    __syncthreads();
    if (threadIdx.x == 0) {
        p->chained = carry;
        p->removed = s_removed;
    }
}

__global__ __launch_bounds__(kBpThreads) void bp_gather_kernel(const unsigned *seg, const unsigned *count,
                                                                const unsigned *offset, unsigned *list)
{
    const unsigned c = count[blockIdx.x];
    if (c == 0) return;
    const unsigned o = offset[blockIdx.x];
    const int64_t base = (int64_t)blockIdx.x * kBpChunk;
    for (unsigned j = threadIdx.x; j < c; j += kBpThreads) list[o + j] = seg[base + j];
}

// The chained pixels (list in index order) in one workgroup, in rounds.  A chained pixel depends on the row above
// and on its left neighbour only, so a round takes list entries [s, e) up to the first entry whose row directly
// follows the previous entry's row: within a round no two rows are adjacent.  Every run of consecutive indices in
// the round is walked left to right by one lane (the replaced left neighbour kept in a register), the runs side by
// side; a barrier between rounds.  A sparse list (a natural frame) takes a few rounds, a hot column one per row.
// A single workgroup: no ordering between workgroups is needed.
__global__ __launch_bounds__(kWalkThreads) void bp_walk_kernel(float *data, int width, const unsigned *list,
                                                                const BpParams *p)
{
    __shared__ unsigned s_end;
    const unsigned m = p->chained;
    unsigned s = 0;
    while (s < m) {
        unsigned e = m;
        for (unsigned c0 = s + 1; c0 < m; c0 += kWalkThreads) {
            if (threadIdx.x == 0) s_end = m;
            __syncthreads();
            const unsigned k = c0 + threadIdx.x;
            const bool next_row = k < m && list[k] / (unsigned)width == list[k - 1] / (unsigned)width + 1;
            const unsigned long long b = __ballot(next_row);          // (one LDS atomic per wave: a hot column puts
            if ((threadIdx.x & 63) == 0 && b)                          //  a row change on every entry of the chunk)
                atomicMin(&s_end, k + (unsigned)__ffsll((long long)b) - 1u);
            __syncthreads();
            const unsigned f = s_end;
            __syncthreads();                                // (s_end is reset by the next chunk)
            if (f < m) { e = f; break; }
        }
        for (unsigned k0 = s + threadIdx.x; k0 < e; k0 += kWalkThreads) {
            unsigned k = k0, i = list[k];
            if (k != s && list[k - 1] == i - 1) continue;   // not the start of a run
            float left = data[i - 1];                       // final: not chained, or chained in an earlier round
            for (;;) {
                const float *r0 = data + i - width, *r1 = data + i, *r2 = data + i + width;
                const float med = median9(r0[-1], r0[0], r0[1], left, r1[0], r1[1], r2[-1], r2[0], r2[1]);
                data[i] = med;
                left = med;
                if (++k >= e || list[k] != i + 1) break;
                i++;
            }
        }
        __syncthreads();
        s = e;
    }
}

}  // namespace

hipError_t launch_calibrate(const float *in, float *out, int64_t n, const float *dark, const float *flat,
                            float flat_max, hipStream_t stream)
{
    auto aligned = [](const float *q) { return q == nullptr || ((uintptr_t)q & 15) == 0; };
    const bool vec = aligned(in) && aligned(out) && aligned(dark) && aligned(flat);
    const int64_t items = vec ? (n >> 2) : n;
    int64_t grid = (items + 255) / 256;
    if (grid > 8192) grid = 8192;
    if (grid < 1) grid = 1;
    Launcher L(stream);
    with_bool(dark != nullptr, [&](auto D) {
        with_bool(flat != nullptr, [&](auto F) {
            with_bool(vec, [&](auto V) {
                L(calibrate_kernel<decltype(D)::value, decltype(F)::value, decltype(V)::value>, (unsigned)grid, 256, 0,
                  in, out, n, dark, flat, flat_max);
            });
        });
    });
    return L.err;
}

int bp_blocks(int64_t n) { return (int)((n + kBpChunk - 1) / kBpChunk); }

hipError_t launch_badpixel(float *data, int width, int height, float sigma_low, float sigma_high, const BpScratch &s,
                           hipStream_t stream)
{
    const int64_t n = (int64_t)width * height;
    const int blocks = bp_blocks(n);
    Launcher L(stream);
    L(bp_diff_kernel, s.stat_blocks, kBpThreads, 0, data, s.diff, width, height, s.partial);
    L(bp_mean_kernel, 1, kBpThreads, 0, s.partial, s.stat_blocks, n, s.params);
    L(bp_variance_kernel, s.stat_blocks, kBpThreads, 0, s.diff, n, s.params, s.partial);
    L(bp_threshold_kernel, 1, kBpThreads, 0, s.partial, s.stat_blocks, n, sigma_low, sigma_high, s.params);
    L(bp_classify_kernel, blocks, kBpThreads, 0, data, s.diff, width, height, s.params, s.seg, s.count, s.removed);
    L(bp_scan_kernel, 1, kScanThreads, 0, s.count, s.removed, s.offset, blocks, s.params);
    L(bp_gather_kernel, blocks, kBpThreads, 0, s.seg, s.count, s.offset, s.list);
    L(bp_walk_kernel, 1, kWalkThreads, 0, data, width, s.list, s.params);
    return L.err;
}

}  // namespace nl
