// stars.hip -- star detection for gfx950: star.FindStars (internal/star/findstars.go:59-103), bit-exact.
//
// Stages, all on one stream:
//   star_scan        findBrightPixels (:105-131).  One wave per row: the candidate chain only couples pixels of one row
//                    (oldS.Y == is.Y), so each wave ballots the pixels above the threshold and walks the row's chain over
//                    the hits, wave-uniformly.  The row's candidates go to a segment of ceil(width / (radius+1)) entries
//                    (appended candidates lie more than radius apart); the wave also flags +-Inf.       (R 4 B / pixel)
//   star_offsets, star_compact   the segments -> one list in row-major (= the reference's) order
//   star_std_*       deviation 1, only when bp_sigma > 0 and MedianDiffStats is nil: Stats.StdDev's arithmetic over
//                    data[i] - median9(1-D mask) for every pixel whose mask lies inside the data
//   star_reject      rejectBadPixels (:134-168): one lane per candidate whose mask lies inside the data
//   star_reject_edge one lane walks the candidates whose mask leaves the data, in list order: GatherAndMedian fills
//                    only the slots it can, and the network runs over the whole buffer with the previous candidate's
//                    leftovers in the rest (the buffer starts zeroed)
//   (host)           QSortStarsDesc (qsort.go:25-57) and filterOutOverlaps (:209-270), literally: order-dependent,
//                    over a short list, with the reference's panics turned into errors
//   star_centroid    shiftToCenterOfMass (:274-325): one lane per star, the fp32 sums in the reference's order
//   (host)           sort and filter again
//   star_hfr         calcAndFilterHalfFluxRadius (:327-383): one lane per star; the compaction and the two serial
//                    sums (sumOfShifts, avgHFR) run on the host over the short list
// Go's float -> int32 conversion is CVTTSS2SL / CVTTSD2SL on amd64: truncation, and 0x80000000 for NaN or out of range
// (go_i32).  Index arithmetic is int32 with wrap-around (wrap_add / wrap_mul), as in Go.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "frame_common.hpp"
#include "launch_common.hpp"
#include "median9.hpp"
#include "stars.hpp"

namespace nl {

namespace {

constexpr int kScanThreads = 256;      // four rows per workgroup
constexpr int kRejectThreads = 256;
constexpr int kStarThreads = 64;
constexpr int kStdThreads = 256;

__host__ __device__ inline int32_t wrap_add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
__host__ __device__ inline int32_t wrap_mul(int32_t a, int32_t b) { return (int32_t)((uint32_t)a * (uint32_t)b); }

struct DevStar {                       // = nl_star_t
    int32_t index;
    float value, x, y, mass, hfr;
};
static_assert(sizeof(DevStar) == sizeof(nl_star_t), "DevStar mirrors nl_star_t");

__global__ __launch_bounds__(kScanThreads) void star_scan_kernel(const float *data, int width, int height, float thr,
                                                                  int radius, int cap, uint2 *seg, unsigned *rowcnt,
                                                                  unsigned *flags)
{
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * (kScanThreads / 64) + (threadIdx.x >> 6);
    if (y >= height) return;
    const float *row = data + (int64_t)y * width;
    uint2 *out = seg + (int64_t)y * cap;
    const int32_t rowbase = y * width;
    int cnt = 0, lx = 0;                 // candidates of the row so far; the last one's x and value (wave-uniform)
    float lv = 0.0f;
    bool inf = false;
    for (int base = 0; base < width; base += 256) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = base + 64 * k + lane;
            v[k] = x < width ? row[x] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int x = base + 64 * k + lane;
            inf |= x < width && isinf(v[k]);
            uint64_t m = __ballot(x < width && v[k] > thr);     // a NaN pixel is never a candidate
            while (m) {
                const int b = __ffsll((unsigned long long)m) - 1;
                m &= m - 1;
                const float hv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), b));
                const int hx = base + 64 * k + b;
                if (cnt > 0 && lx >= hx - radius) {              // oldS.X >= is.X - radius on the same row
                    if (!(lv >= hv)) { lx = hx; lv = hv; }       // replace with the brighter one, else keep
                } else {
                    if (cnt > 0 && cnt <= cap && lane == 0) out[cnt - 1] = make_uint2((unsigned)(rowbase + lx), __float_as_uint(lv));
                    cnt++;
                    lx = hx;
                    lv = hv;
                }
            }
        }
    }
    if (lane == 0) {
        if (cnt > 0 && cnt <= cap) out[cnt - 1] = make_uint2((unsigned)(rowbase + lx), __float_as_uint(lv));
        rowcnt[y] = (unsigned)min(cnt, cap);
    }
    if (__any(inf) && lane == 0) atomicOr(flags, 1u);
}

// rowcnt[0 .. height) -> exclusive offsets, rowcnt[height] = the total (one workgroup)
__global__ __launch_bounds__(1024) void star_offsets_kernel(unsigned *rowcnt, int height)
{
    __shared__ unsigned s[1024];
    const int t = threadIdx.x;
    const int per = (height + 1023) / 1024;
    const int lo = min(t * per, height), hi = min(lo + per, height);
    unsigned sum = 0;
    for (int y = lo; y < hi; y++) sum += rowcnt[y];
    s[t] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        const unsigned v = t >= off ? s[t - off] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    unsigned run = s[t] - sum;
    for (int y = lo; y < hi; y++) {
        const unsigned c = rowcnt[y];
        rowcnt[y] = run;
        run += c;
    }
    if (t == 1023) rowcnt[height] = s[1023];
}

__global__ __launch_bounds__(kScanThreads) void star_compact_kernel(const uint2 *seg, const unsigned *off, int height,
                                                                     int cap, uint2 *list)
{
    const int lane = threadIdx.x & 63;
    const int y = blockIdx.x * (kScanThreads / 64) + (threadIdx.x >> 6);
    if (y >= height) return;
    const unsigned o = off[y], c = off[y + 1] - o;
    for (unsigned k = lane; k < c; k += 64) list[o + k] = seg[(int64_t)y * cap + k];
}

// data[i] - MedianFloat32Slice9 of the CreateMask(width, 1.5) gather (findstars.go:187-200, gather.go:26-38), for a
// pixel whose whole mask lies inside the data: row above, own row, row below, each left to right (1-D offsets)
__device__ __forceinline__ float star_med(const float *d, int64_t i, int w)
{
    return median9_cmp(d[i - w - 1], d[i - w], d[i - w + 1], d[i - 1], d[i], d[i + 1], d[i + w - 1], d[i + w],
                       d[i + w + 1]);
}
__device__ __forceinline__ float star_med_diff(const float *d, int64_t i, int w) { return d[i] - star_med(d, i, w); }

// Stats.Mean (stats.go:264-277): the fp64 sum of the differences over [lo, hi)
__global__ __launch_bounds__(kStdThreads) void star_std_sum_kernel(const float *data, int width, int64_t lo, int64_t hi,
                                                                    double *partial)
{
    double s = 0.0;
    for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (int64_t)gridDim.x * blockDim.x)
        s += (double)star_med_diff(data, i, width);
    s = block_sum<kStdThreads>(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// calcVariance (stats.go:280-287): float64(v - mean)^2 summed in fp64
__global__ __launch_bounds__(kStdThreads) void star_std_var_kernel(const float *data, int width, int64_t lo, int64_t hi,
                                                                    const float *params, double *partial)
{
    const float mean = params[0];
    double s = 0.0;
    for (int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (int64_t)gridDim.x * blockDim.x) {
        const double d = (double)(star_med_diff(data, i, width) - mean);
        s += d * d;
    }
    s = block_sum<kStdThreads>(s);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// one workgroup: step 0 mean = float32(sum / m) -> params[0]; step 1 std = float32(sqrt(var / m)) -> params[1],
// threshold std * sigma (rejectBadPixels, findstars.go:157) -> params[2]
__global__ __launch_bounds__(kStdThreads) void star_std_final_kernel(const double *partial, int blocks, int64_t m,
                                                                      float sigma, int step, float *params)
{
    double s = 0.0;
    for (int b = threadIdx.x; b < blocks; b += kStdThreads) s += partial[b];
    s = block_sum<kStdThreads>(s);
    if (threadIdx.x == 0) {
        if (step == 0) {
            params[0] = (float)(s / (double)m);
        } else {
            const float std = (float)sqrt(s / (double)m);
            params[1] = std;
            params[2] = std * sigma;
        }
    }
}

__device__ __forceinline__ bool star_keep(float v, float med, float t)
{
    const float diff = v - med;
    return diff < t && -diff < t;
}

// candidates whose mask lies inside the data: one lane each
__global__ __launch_bounds__(kRejectThreads) void star_reject_kernel(const float *data, int width, int64_t n,
                                                                      const uint2 *list, const unsigned *total,
                                                                      const float *params, float t_given,
                                                                      unsigned char *keep)
{
    const float t = params ? params[2] : t_given;
    const unsigned cnt = *total;
    for (unsigned k = blockIdx.x * blockDim.x + threadIdx.x; k < cnt; k += gridDim.x * blockDim.x) {
        const int64_t i = list[k].x;
        if (i >= width + 1 && i <= n - width - 2) keep[k] = star_keep(data[i], star_med(data, i, width), t);
    }
}

// GatherAndMedian into the shared buffer a (gather.go:26-38): the offsets inside [0, n) fill a[0 ..), in mask order
__device__ void star_gather(const float *data, int width, int64_t n, int64_t i, float (&a)[9])
{
    const int64_t off[9] = {-(int64_t)width - 1, -(int64_t)width, -(int64_t)width + 1, -1, 0, 1,
                            (int64_t)width - 1, (int64_t)width, (int64_t)width + 1};
    int num = 0;
    for (int j = 0; j < 9; j++) {
        const int64_t io = i + off[j];
        if (io >= 0 && io < n) a[num++] = data[io];
    }
}

// the candidates whose mask leaves the data -- a prefix (index < width + 1) and a suffix (index > n - width - 2) of the
// list -- in list order, through one buffer: zeroed at the start, and before the suffix the final buffer of the
// candidate in front of it (an interior one, whose gather fills every slot, or the prefix's last)
__global__ void star_reject_edge_kernel(const float *data, int width, int64_t n, const uint2 *list,
                                        const unsigned *total, const float *params, float t_given, unsigned char *keep)
{
    if (threadIdx.x != 0) return;
    const float t = params ? params[2] : t_given;
    const unsigned cnt = *total;
    unsigned p = 0, q = cnt;
    while (p < cnt && (int64_t)list[p].x < width + 1) p++;
    while (q > p && (int64_t)list[q - 1].x > n - width - 2) q--;
    float a[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (unsigned k = 0; k < p; k++) {
        const int64_t i = list[k].x;
        star_gather(data, width, n, i, a);
        keep[k] = star_keep(data[i], median9_cmp_buf(a), t);
    }
    if (q < cnt && q > p) {
        star_gather(data, width, n, list[q - 1].x, a);
        (void)median9_cmp_buf(a);
    }
    for (unsigned k = q; k < cnt; k++) {
        const int64_t i = list[k].x;
        star_gather(data, width, n, i, a);
        keep[k] = star_keep(data[i], median9_cmp_buf(a), t);
    }
}

// shiftToCenterOfMass (findstars.go:274-325) for one star per lane
__global__ __launch_bounds__(kStarThreads) void star_centroid_kernel(const float *data, int width, int64_t n, float thr,
                                                                      int radius, const DevStar *in, int count,
                                                                      DevStar *out, float *shift)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    DevStar s = in[i];
    float shift_sq = 3.40282346638528859811704183484516925440e+38f;      // math.MaxFloat32
    for (int round = 0; shift_sq > 0.0001f && round < 10; round++) {
        float xm = 0.0f, ym = 0.0f, mass = 0.0f;
        for (int y = -radius; y <= radius; y++) {
            const int32_t rb = wrap_add(s.index, wrap_mul(y, width));
            const float fy = (float)y;
            for (int x = -radius; x <= radius; x++) {
                const int32_t idx = wrap_add(rb, x);
                float value = 0.0f;
                if (idx >= 0 && (int64_t)idx < n) {
                    value = data[idx] - thr;
                    if (value < 0.0f) value = 0.0f;
                }
                xm += (float)x * value;
                ym += fy * value;
                mass += value;
            }
        }
        const int32_t x0 = s.index % width, y0 = s.index / width;
        if (mass == 0.0f) mass = 1e-8f;
        const float dx = xm / mass, dy = ym / mass;
        const float nx = (float)x0 + dx, ny = (float)y0 + dy;
        const float pdx = nx - s.x, pdy = ny - s.y;
        shift_sq = pdx * pdx + pdy * pdy;
        const int32_t idx = wrap_add(wrap_add(s.index, wrap_mul(width, go_i32(dy + 0.5f))), go_i32(dx + 0.5f));
        const float value = (idx >= 0 && (int64_t)idx < n) ? data[idx] : 0.0f;
        s = DevStar{idx, value, nx, ny, mass, 0.0f};
    }
    out[i] = s;
    shift[i] = (float)sqrt((double)shift_sq);
}

// calcAndFilterHalfFluxRadius (findstars.go:327-383) for one star per lane: HFR and mass into out, keep[i]
__global__ __launch_bounds__(kStarThreads) void star_hfr_kernel(const float *data, int width, int64_t n, float radius,
                                                                 int rad, int dist_sq_limit, float location,
                                                                 float star_in_out, DevStar *stars, int count,
                                                                 unsigned char *keep)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    DevStar s = stars[i];
    float moment = 0.0f, mass = 0.0f;
    int32_t pixels = 0;
    for (int y = -rad; y <= rad; y++) {
        const int32_t rb = wrap_add(s.index, wrap_mul(y, width));
        for (int x = -rad; x <= rad; x++) {
            const int32_t dsq = x * x + y * y;
            if (dsq > dist_sq_limit) continue;
            const float distance = (float)sqrt((double)dsq);
            const int32_t idx = wrap_add(rb, x);
            float value = 0.0f;
            if (idx >= 0 && (int64_t)idx < n) {
                const float v = data[idx] - location;
                if (v > 0.0f) value = v;                 // (NaN: 0)
            }
            moment += distance * value;
            mass += value;
            pixels++;
        }
    }
    if (mass == 0.0f) mass = 1e-8f;
    const float hfr = moment / mass;
    bool k = false;
    if (!(hfr > radius)) {
        // (a NaN hfr gives innerRad = MinInt32: the reference's one pass of the loops is skipped, as none runs here)
        const int64_t inner_rad = go_i32(ceil((double)hfr));
        const int32_t lim = go_i32(ceil((double)(hfr * hfr)));
        float inner_mass = 0.0f;
        int32_t inner_pixels = 0;
        for (int64_t y = -inner_rad; y <= inner_rad; y++) {
            const int32_t rb = wrap_add(s.index, wrap_mul((int32_t)y, width));
            for (int64_t x = -inner_rad; x <= inner_rad; x++) {
                const int32_t dsq = (int32_t)(x * x + y * y);
                if (dsq > lim) continue;
                const int32_t idx = wrap_add(rb, (int32_t)x);
                float value = 0.0f;
                if (idx >= 0 && (int64_t)idx < n) {
                    const float v = data[idx] - location;
                    if (v > 0.0f) value = v;
                }
                inner_mass += value;
                inner_pixels++;
            }
        }
        const float outer_mass = mass - inner_mass;
        const int32_t outer_pixels = pixels - inner_pixels;
        k = !(inner_mass * (float)outer_pixels <= star_in_out * outer_mass * (float)inner_pixels);
    }
    s.hfr = hfr;
    s.mass = mass;
    stars[i] = s;
    keep[i] = k;
}

// ---- host: the order-dependent steps over the short list ----

struct Panic {
    const char *site;
};

// QPartitionStarsDesc (qsort.go:37-57) on a[lo, hi): Hoare's partition around the middle element's Mass.  The scans
// are bounds-checked: a NaN pivot lets them run off the slice, where the reference panics.
static bool partition_desc(nl_star_t *a, int64_t lo, int64_t hi, int64_t *out)
{
    const int64_t len = hi - lo;
    const int64_t mid = (len - 1) >> 1;
    const float pivot = a[lo + mid].mass;
    int64_t l = -1, r = len;
    for (;;) {
        for (;;) {
            l++;
            if (l >= len) return false;
            if (a[lo + l].mass <= pivot) break;
        }
        for (;;) {
            r--;
            if (r < 0) return false;
            if (a[lo + r].mass >= pivot) break;
        }
        if (l >= r) {
            *out = r;
            return true;
        }
        std::swap(a[lo + l], a[lo + r]);
    }
}

// QSortStarsDesc (qsort.go:25-33) with an explicit stack: a[:index+1] and a[index+1:] are disjoint, so the order in which
// they are sorted does not matter
static bool qsort_desc(std::vector<nl_star_t> &a)
{
    std::vector<std::pair<int64_t, int64_t>> todo;
    todo.emplace_back(0, (int64_t)a.size());
    while (!todo.empty()) {
        const auto seg = todo.back();
        todo.pop_back();
        if (seg.second - seg.first <= 1) continue;
        int64_t idx;
        if (!partition_desc(a.data(), seg.first, seg.second, &idx)) return false;
        todo.emplace_back(seg.first + idx + 1, seg.second);
        todo.emplace_back(seg.first, seg.first + idx + 1);
    }
    return true;
}

static int32_t go_div(int32_t a, int32_t b) { return (a == INT32_MIN && b == -1) ? INT32_MIN : a / b; }

// filterOutOverlaps (findstars.go:209-270): a 256-pixel grid of per-cell lists in insertion order; a star is kept unless
// a kept star in its own or an adjacent cell lies within the radius.  A cell index outside the grid panics there.
static bool filter_overlaps(std::vector<nl_star_t> &stars, int32_t width, int32_t height, int32_t radius)
{
    const int32_t bin = 256;
    const int32_t xbins = (width + bin - 1) / bin, ybins = (height + bin - 1) / bin;
    std::vector<std::vector<int32_t>> bins((size_t)xbins * (size_t)ybins);
    const int32_t r2 = wrap_mul(radius, radius);
    size_t kept = 0;
    for (size_t i = 0; i < stars.size(); i++) {
        const nl_star_t s = stars[i];
        const int32_t xc = go_div(go_i32(s.x + 0.5f), bin), yc = go_div(go_i32(s.y + 0.5f), bin);
        bool near = false;
        for (int32_t dy = -1; dy <= 1 && !near; dy++) {
            if (yc + dy < 0 || yc + dy >= ybins) continue;
            for (int32_t dx = -1; dx <= 1 && !near; dx++) {
                if (xc + dx < 0 || xc + dx >= xbins) continue;
                for (const int32_t j : bins[(size_t)((xc + dx) + (yc + dy) * xbins)]) {
                    const float xd = s.x - stars[j].x, yd = s.y - stars[j].y;
                    const float sq = xd * xd + yd * yd;
                    if (go_i32(sq + 0.5f) <= r2) {
                        near = true;
                        break;
                    }
                }
            }
        }
        if (near) continue;
        stars[kept] = s;
        const int32_t cell = wrap_add(xc, wrap_mul(yc, xbins));
        if (cell < 0 || (size_t)cell >= bins.size()) return false;
        bins[(size_t)cell].push_back((int32_t)kept);
        kept++;
    }
    stars.resize(kept);
    return true;
}

static const char *kPanicSort = "QPartitionStarsDesc (qsort.go:37-57) would index past the slice: a star's Mass is NaN";
static const char *kPanicBins = "filterOutOverlaps (findstars.go:250-256) would index bins out of range: a star's "
                                "centroid lies outside the bin grid (NaN position, or pulled past the last cell)";

}  // namespace

int find_stars_run(const float *d_data, int width, int height, const StarParams &p, StarWork &w, double *d_partial,
                   int stat_blocks, hipStream_t stream, std::vector<nl_star_t> &stars, float *sum_of_shifts,
                   float *avg_hfr, std::string *msg)
{
    const int64_t n = (int64_t)width * height;
    const int r = p.radius;
    const int cap = (int)(((int64_t)width + r) / ((int64_t)r + 1));       // ceil(width / (radius + 1)) >= 1
    const size_t maxc = (size_t)height * (size_t)cap;
    uint2 *seg, *list;
    unsigned char *keep;
    unsigned *rowcnt, *flags;
    float *params;
    auto carve = [&](void *base) {
        Carver c(base);
        seg = c.take<uint2>(maxc);
        list = c.take<uint2>(maxc);
        keep = c.take<unsigned char>(maxc);
        rowcnt = c.take<unsigned>((size_t)height + 1);
        flags = c.take<unsigned>(1);
        params = c.take<float>(3);
        return align_up(c.bytes());
    };
    NL_RUN_HIP(w.buf.reserve(carve(nullptr), stream));
    carve(w.buf.ptr);

    // findBrightPixels (:105-131), threshold location + scale*starSig in fp32 (:61)
    const float thr = p.location + p.scale * p.star_sig;
    NL_RUN_HIP(hipMemsetAsync(flags, 0, sizeof(unsigned), stream));
    const int rows_grid = (height + kScanThreads / 64 - 1) / (kScanThreads / 64);
    Launcher L(stream);
    L(star_scan_kernel, rows_grid, kScanThreads, 0, d_data, width, height, thr, r, cap, seg, rowcnt, flags);
    L(star_offsets_kernel, 1, 1024, 0, rowcnt, height);
    L(star_compact_kernel, rows_grid, kScanThreads, 0, seg, rowcnt, height, cap, list);
    NL_RUN_LAUNCHED(L);

    // rejectBadPixels (:134-168)
    const bool bp = p.bp_sigma > 0.0f;
    const unsigned *total = rowcnt + height;
    if (bp) {
        const float *tp = nullptr;
        float t_given = 0.0f;
        if (isnan(p.diff_std)) {      // deviation 1: every pixel whose whole mask lies inside the data
            const int64_t lo = (int64_t)width + 1, hi = std::max(lo, n - width - 1), m = hi - lo;
            const int64_t want = (m + kStdThreads - 1) / kStdThreads;
            const int g = (int)std::max<int64_t>(1, std::min<int64_t>(want, stat_blocks));
            L(star_std_sum_kernel, g, kStdThreads, 0, d_data, width, lo, hi, d_partial);
            L(star_std_final_kernel, 1, kStdThreads, 0, d_partial, g, m, p.bp_sigma, 0, params);
            L(star_std_var_kernel, g, kStdThreads, 0, d_data, width, lo, hi, params, d_partial);
            L(star_std_final_kernel, 1, kStdThreads, 0, d_partial, g, m, p.bp_sigma, 1, params);
            tp = params;
        } else {
            t_given = p.diff_std * p.bp_sigma;
        }
        const int g = (int)std::min<size_t>((maxc + kRejectThreads - 1) / kRejectThreads, 4096);
        L(star_reject_kernel, g, kRejectThreads, 0, d_data, width, n, list, total, tp, t_given, keep);
        L(star_reject_edge_kernel, 1, 64, 0, d_data, width, n, list, total, tp, t_given, keep);
        NL_RUN_LAUNCHED(L);
    }
    unsigned head[2] = {0, 0};
    NL_RUN_HIP(hipMemcpyAsync(&head[0], total, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    NL_RUN_HIP(hipMemcpyAsync(&head[1], flags, sizeof(unsigned), hipMemcpyDeviceToHost, stream));
    NL_RUN_HIP(hipStreamSynchronize(stream));
    if (head[1] & 1u) {
        *msg = "find_stars: the frame holds +-Inf (not supported)";
        return NL_ERR_INVALID_ARG;
    }
    const size_t cnt = head[0];
    std::vector<uint2> cand(cnt);
    std::vector<unsigned char> kept(bp ? cnt : 0);
    if (cnt) {
        NL_RUN_HIP(hipMemcpyAsync(cand.data(), list, sizeof(uint2) * cnt, hipMemcpyDeviceToHost, stream));
        if (bp) NL_RUN_HIP(hipMemcpyAsync(kept.data(), keep, cnt, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipStreamSynchronize(stream));
    }
    stars.clear();
    stars.reserve(cnt);
    for (size_t k = 0; k < cnt; k++) {
        if (bp && !kept[k]) continue;
        const int32_t idx = (int32_t)cand[k].x;
        float v;
        memcpy(&v, &cand[k].y, sizeof v);
        // Star{Index, Value, X: int32(i) % width, Y: int32(i) / width, Mass: v, HFR: 1} (:109)
        stars.push_back(nl_star_t{idx, v, (float)(idx % width), (float)(idx / width), v, 1.0f});
    }

    // QSortStarsDesc + filterOutOverlaps (:74-76)
    if (!qsort_desc(stars)) { *msg = kPanicSort; return NL_ERR_INVALID_ARG; }
    if (!filter_overlaps(stars, width, (int32_t)(n / width), r)) { *msg = kPanicBins; return NL_ERR_INVALID_ARG; }

    // shiftToCenterOfMass (:79), threshold location + scale*starSig*0.5
    const int m1 = (int)stars.size();
    DevStar *d_in, *d_out;
    float *d_shift;
    auto carve_stars = [&](void *base) {
        Carver c(base);
        d_in = c.take<DevStar>((size_t)m1);
        d_out = c.take<DevStar>((size_t)m1);
        d_shift = c.take<float>((size_t)m1);
        c.take<char>(1);                  // (no star: still an allocation)
        return align_up(c.bytes());
    };
    NL_RUN_HIP(w.stars.reserve(carve_stars(nullptr), stream));
    carve_stars(w.stars.ptr);
    float sum = 0.0f;
    if (m1) {
        const float thr2 = p.location + p.scale * p.star_sig * 0.5f;
        NL_RUN_HIP(hipMemcpyAsync(d_in, stars.data(), sizeof(DevStar) * (size_t)m1, hipMemcpyHostToDevice, stream));
        L(star_centroid_kernel, (m1 + kStarThreads - 1) / kStarThreads, kStarThreads, 0, d_data, width, n, thr2, r, d_in,
          m1, d_out, d_shift);
        NL_RUN_LAUNCHED(L);
        std::vector<float> shift((size_t)m1);
        NL_RUN_HIP(hipMemcpyAsync(stars.data(), d_out, sizeof(DevStar) * (size_t)m1, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipMemcpyAsync(shift.data(), d_shift, sizeof(float) * (size_t)m1, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipStreamSynchronize(stream));
        for (int i = 0; i < m1; i++) sum += shift[(size_t)i];      // sumOfShifts, in list order (:322)
    }

    if (!qsort_desc(stars)) { *msg = kPanicSort; return NL_ERR_INVALID_ARG; }
    if (!filter_overlaps(stars, width, (int32_t)(n / width), r)) { *msg = kPanicBins; return NL_ERR_INVALID_ARG; }

    // calcAndFilterHalfFluxRadius (:88) with float32(radius)
    const int m2 = (int)stars.size();
    float avg = 0.0f;
    size_t nk = 0;
    if (m2) {
        const float rf = (float)r;
        const int rad = go_i32(ceil((double)rf));
        const float re = rf + 1e-8f;
        const int lim = go_i32(ceil((double)re * (double)re));
        unsigned char *d_keep = reinterpret_cast<unsigned char *>(d_out);
        NL_RUN_HIP(hipMemcpyAsync(d_in, stars.data(), sizeof(DevStar) * (size_t)m2, hipMemcpyHostToDevice, stream));
        L(star_hfr_kernel, (m2 + kStarThreads - 1) / kStarThreads, kStarThreads, 0, d_data, width, n, rf, rad, lim,
          p.location, p.star_in_out, d_in, m2, d_keep);
        NL_RUN_LAUNCHED(L);
        std::vector<unsigned char> hk((size_t)m2);
        NL_RUN_HIP(hipMemcpyAsync(stars.data(), d_in, sizeof(DevStar) * (size_t)m2, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipMemcpyAsync(hk.data(), d_keep, (size_t)m2, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipStreamSynchronize(stream));
        for (int i = 0; i < m2; i++) {
            if (!hk[(size_t)i]) continue;
            stars[nk++] = stars[(size_t)i];
            avg += stars[(size_t)i].hfr;
        }
    }
    stars.resize(nk);
    avg /= (float)nk;                 // (no stars: 0/0 = NaN, as the reference)
    *sum_of_shifts = sum;
    *avg_hfr = avg;
    return NL_OK;
}

}  // namespace nl
