// background.hip -- background extraction for gfx950: OpBackExtract (internal/ops/pre/preprocess.go:372-398), i.e.
// pre.NewBackground (background.go:68-106) and Background.Subtract / Render (:309-462), bit-exact.
//
// Stages, all on one stream:
//   (host)          grid geometry (:72-78) and binStarsIntoCells (:108-143), literally, into one star list per cell
//                   with hfrSq = ((HFR*HFR)*f)*f precomputed as gatherWithoutStars forms it (:507)
//   back_fit        FitCell (:464-492) for every cell, one workgroup per cell.  The workgroup gathers the star-masked
//                   pixels of its cell (in LDS when the cell fits, else into a global staging area re-read by every
//                   pass) and computes the three QSelectMedianFloat32 results as order statistics: a radix select over
//                   order-preserving uint32 keys, 8 bits per pass, histograms in LDS.  An even count takes `lower` as
//                   the (k-1)-th order statistic (one count and one max-reduction below the k-th key).  The MAD set and
//                   the trimmed set are formed on the fly from the gathered samples.  For NaN-free samples each result
//                   is a function of the multiset only, so the reference's in-place reordering cannot change it (up to
//                   the sign of a zero tied at the median rank).  A cell with a NaN sample, or with a non-finite median
//                   (the MAD set would hold a NaN), depends on the order: the kernel flags it for the host.
//   (host)          flagged cells: the literal QSelect* over the samples in gather order, from a download of the cell's
//                   rectangle; then clip / interpolate (:175-200, :256-306), gauss3x3 (:203-239), calculateStats
//                   (:241-254), and the two state machines of Subtract (:386-462) as per-column / per-row tables
//   back_subtract   data[i] -= v, v the bilinear value in the reference's fp32 order; optionally also writes v (Render)
// The reference's panics (empty selections, out-of-range indices, a NaN pivot) and its one endless loop come back as
// NL_ERR_INVALID_ARG with a message naming the site.
#include <float.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "background.hpp"
#include "frame_common.hpp"
#include "launch_common.hpp"
#include "select_common.hpp"

namespace nl {

namespace {

constexpr int kFitThreads = kSelectThreads;     // four waves per cell (the select of select_common.hpp)
constexpr int kSubThreads = 256;
constexpr int kSubCols = 4;            // columns per lane of back_subtract
constexpr size_t kLdsCap = 80 * 1024;  // LDS of one cell's workgroup: two workgroups per CU (160 KiB)

enum CellStatus : int { kCellOk = 0, kCellHost = 1, kCellEmpty = 2, kCellEmptyTrim = 3 };

using FitShared = SelectShared;

// QSelectMedianFloat32 (qsort.go:68-82) of the `members` members as an order statistic
template <class Get>
__device__ float block_median(int n, unsigned members, Get get, FitShared &sh)
{
    const unsigned k = (members >> 1) + 1;
    const uint32_t uk = block_select(n, k, get, sh);
    const float upper = key2f(uk);
    if (members & 1) return upper;
    unsigned below = 0, top = 0;
    for (int i = threadIdx.x; i < n; i += kFitThreads) {
        uint32_t key;
        if (get(i, &key) && key < uk) { below++; top = max(top, key); }
    }
    below = block_sum(below, sh.red);
    top = block_max(top, sh.red);
    const float lower = below < k - 1 ? upper : key2f(top);
    return 0.5f * (lower + upper);
}

// FitCell (background.go:464-492) of one cell per workgroup.  rect: xStart, xEnd, yStart, yEnd; the cell's stars are
// mstar[star_off[c] .. star_off[c+1]) = (X, Y, hfrSq).  kLds: the samples live in LDS (dynamic, after FitShared), else
// at stage[yStart*width + xStart*(yEnd-yStart)] (the cells tile the image, so the areas never overlap).
template <bool kLds>
__global__ __launch_bounds__(kFitThreads) void back_fit_kernel(const float *data, int width, const int4 *rect,
                                                               const int *star_off, const float4 *mstar, float sigma,
                                                               float *stage, float *cell_val, int *cell_n,
                                                               int *cell_status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    FitShared &sh = *reinterpret_cast<FitShared *>(lds);
    const int c = blockIdx.x;
    const int4 r = rect[c];
    const int cw = r.y - r.x, area = cw * (r.w - r.z);
    float *vals = kLds ? reinterpret_cast<float *>(lds + ((sizeof(FitShared) + 15) & ~(size_t)15))
                       : stage + ((int64_t)r.z * width + (int64_t)r.x * (r.w - r.z));
    const int s0 = star_off[c], s1 = star_off[c + 1];
    if (threadIdx.x == 0) { sh.count = 0; sh.nan = 0; }
    __syncthreads();

    // gatherWithoutStars (:494-515); the order of the gathered samples does not matter here
    const int lane = threadIdx.x & 63;
    for (int base = 0; base < area; base += kFitThreads) {
        const int i = base + threadIdx.x;
        bool keep = false;
        float v = 0.0f;
        if (i < area) {
            const int x = r.x + i % cw, y = r.z + i / cw;
            keep = true;
            for (int s = s0; s < s1; s++) {
                const float4 st = mstar[s];
                const float dx = (float)x - st.x, dy = (float)y - st.y;
                const float dist_sq = dx * dx + dy * dy;
                if (dist_sq <= st.z) { keep = false; break; }
            }
            if (keep) v = data[(int64_t)y * width + x];
        }
        const unsigned long long ball = __ballot(keep);
        unsigned pos = 0;
        if (lane == 0 && ball) pos = atomicAdd(&sh.count, (unsigned)__popcll(ball));
        pos = __shfl(pos, 0, 64);
        if (keep) {
            vals[pos + __popcll(ball & ((1ull << lane) - 1))] = v;
            if (v != v) sh.nan = 1;
        }
    }
    __syncthreads();
    const int n = (int)sh.count;
    const bool has_nan = sh.nan != 0;
    if (threadIdx.x == 0) cell_n[c] = n;
    if (n == 0 || has_nan) {
        if (threadIdx.x == 0) { cell_status[c] = n == 0 ? kCellEmpty : kCellHost; cell_val[c] = NAN; }
        return;
    }

    const float median = block_median(n, (unsigned)n, [&](int i, uint32_t *key) { *key = f2key(vals[i]); return true; }, sh);
    if (!isfinite(median)) {           // +-Inf + a sample of the same infinity, or -Inf + Inf: a NaN in the MAD set
        if (threadIdx.x == 0) { cell_status[c] = kCellHost; cell_val[c] = NAN; }
        return;
    }
    const float mad = block_median(n, (unsigned)n, [&](int i, uint32_t *key) {
        *key = f2key(fabsf(vals[i] - median));
        return true;
    }, sh);
    const float std_dev = mad * 1.4826f;
    const float upper_bound = median + sigma * std_dev;

    unsigned kept = 0;
    for (int i = threadIdx.x; i < n; i += kFitThreads) kept += vals[i] < upper_bound;
    kept = block_sum(kept, sh.red);
    if (kept == 0) {
        if (threadIdx.x == 0) { cell_status[c] = kCellEmptyTrim; cell_val[c] = NAN; }
        return;
    }
    const float trimmed = block_median(n, kept, [&](int i, uint32_t *key) {
        const float v = vals[i];
        *key = f2key(v);
        return v < upper_bound;
    }, sh);
    if (threadIdx.x == 0) { cell_status[c] = kCellOk; cell_val[c] = trimmed; }
}

// Subtract (:386-462) / Render (:309-384) per pixel: xl / xr per column, yl*GridCellsX / yr per row from the host's
// state machines (indices checked there).  kVec: width % 4 == 0 and a 16-byte aligned frame.
template <bool kVec, bool kRender>
__global__ __launch_bounds__(kSubThreads) void back_subtract_kernel(float *data, float *bg, int width, int col_blocks,
                                                                    const int *col_xl, const float *col_xr,
                                                                    const int *row_base, const float *row_yr,
                                                                    const float *cells, int cells_x)
{
    const int y = blockIdx.x / col_blocks;
    const int x0 = ((blockIdx.x % col_blocks) * kSubThreads + threadIdx.x) * kSubCols;
    if (x0 >= width) return;
    const int rb = row_base[y];
    const float yr = row_yr[y];
    float *row = data + (int64_t)y * width;
    float in[kSubCols], v[kSubCols];
    if (kVec) {
        const float4 t = *reinterpret_cast<const float4 *>(row + x0);
        in[0] = t.x; in[1] = t.y; in[2] = t.z; in[3] = t.w;
    } else {
        for (int u = 0; u < kSubCols; u++) in[u] = x0 + u < width ? row[x0 + u] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kSubCols; u++) {
        const int x = kVec ? x0 + u : min(x0 + u, width - 1);
        const int xlyl = col_xl[x] + rb;
        const float xr = col_xr[x];
        const float vyl = cells[xlyl] * (1 - xr) + cells[xlyl + 1] * xr;
        const float vyh = cells[xlyl + cells_x] * (1 - xr) + cells[xlyl + 1 + cells_x] * xr;
        v[u] = vyl * (1 - yr) + vyh * yr;
        in[u] -= v[u];
    }
    if (kVec) {
        *reinterpret_cast<float4 *>(row + x0) = make_float4(in[0], in[1], in[2], in[3]);
        if (kRender)
            *reinterpret_cast<float4 *>(bg + (int64_t)y * width + x0) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        for (int u = 0; u < kSubCols && x0 + u < width; u++) {
            row[x0 + u] = in[u];
            if (kRender) bg[(int64_t)y * width + x0 + u] = v[u];
        }
    }
}

static int invalid(std::string *msg, const std::string &m)
{
    *msg = m;
    return NL_ERR_INVALID_ARG;
}

static const char *kPanicSelect = "QSelectFloat32 (qsort.go:94-126) would index past the slice";

// median.MedianFloat32 (median3x3.go:115-119) over at most 8 NaN-free neighbours (never 9)
static float median_f32(float *a, int n)
{
    if (n == 0) return NAN;
    float m = NAN;
    (void)qselect_median_lit(a, n, &m);
    return m;
}

static bool star_eq(const nl_star_t &a, const nl_star_t &b)     // Go's struct ==
{
    return a.index == b.index && a.value == b.value && a.x == b.x && a.y == b.y && a.mass == b.mass && a.hfr == b.hfr;
}

struct Grid {
    int32_t width, height, cells_x, cells_y, cells;
    float sp_x, sp_y;
};

// interpolate (:256-274) with MedianInterpolation (:288-306): the number of changes
static int interpolate(std::vector<float> &p, int32_t w, int32_t h, int neighbors, bool *progress)
{
    static const int off[8][2] = {{-1, -1}, {0, -1}, {1, -1}, {-1, 0}, {1, 0}, {-1, 1}, {0, 1}, {1, 1}};
    float temp[16];
    int changes = 0;
    *progress = false;
    for (int32_t y = 0; y < h; y++)
        for (int32_t x = 0; x < w; x++) {
            const int32_t index = y * w + x;
            if (!isnan(p[index])) continue;
            int got = 0;
            for (const auto &o : off) {
                const int32_t x2 = x + o[0], y2 = y + o[1];
                if (x2 >= 0 && x2 < w && y2 >= 0 && y2 < h) {
                    const float q = p[x2 + y2 * w];
                    if (!isnan(q)) temp[got++] = q;
                }
            }
            const float predict = median_f32(temp, got);
            if (got >= neighbors) {
                p[index] = predict;
                changes++;
                if (!isnan(predict)) *progress = true;
            }
        }
    return changes;
}

static const float kGauss[3] = {0.468592f, 0.107973f, 0.024879f};

// The state machine of Subtract / Render along one axis (:389-400 rows, :401-414 columns): the shifted low cell and
// the fraction of every destination coordinate
static void axis_table(int32_t n, float sp, int32_t cells, int *lo, float *frac)
{
    int32_t src_l = -1, src_h = 0;
    int32_t dest_l = go_i32(-0.5f * sp - 0.5f);
    int32_t dest_h = go_i32(0.5f * sp + 0.5f);
    float span = 1.0f / (float)(dest_h - dest_l);
    for (int32_t d = 0; d < n; d++) {
        if (d >= dest_h) {
            src_l = src_h;
            src_h = src_h + 1;
            dest_l = dest_h;
            dest_h = go_i32(((float)src_h + 0.5f) * sp + 0.5f);
            span = 1.0f / (float)(dest_h - dest_l);
        }
        const float src = (float)src_l + (float)(d - dest_l) * span;
        int32_t l = src_l, h = src_h;
        if (l < 0) { l++; h++; }
        if (h >= cells) { l--; h--; }
        lo[d] = l;
        frac[d] = src - (float)l;
    }
}

}  // namespace

int back_extract_run(float *d_data, int width, int height, const BackParams &p, const nl_star_t *stars, int n_stars,
                     BackWork &w, hipStream_t stream, float *background_host, float *cells_out, int cells_capacity,
                     nl_background_t *info, std::string *msg)
{
    // grid geometry (:72-78)
    Grid g;
    g.width = width;
    g.height = height;
    g.cells_x = (width + p.grid / 2) / p.grid;
    g.cells_y = (height + p.grid / 2) / p.grid;
    if (g.cells_x == 0 || g.cells_y == 0)       // (deviation 2: the reference divides by zero)
        return invalid(msg, "NewBackground (background.go:74-78): " + std::to_string(width) + "x" +
                                std::to_string(height) + " is less than half a grid cell of " + std::to_string(p.grid) +
                                " (grid of " + std::to_string(g.cells_x) + "x" + std::to_string(g.cells_y) + " cells)");
    g.cells = g.cells_x * g.cells_y;
    g.sp_x = (float)width / (float)g.cells_x;
    g.sp_y = (float)height / (float)g.cells_y;
    const int32_t ncell = g.cells;

    // binStarsIntoCells (:108-143): a list of star indices per cell
    std::vector<std::vector<int>> bins(ncell);
    for (int i = 0; i < n_stars; i++) {
        const nl_star_t &s = stars[i];
        const float sx = s.x, sy = s.y, hfr = s.hfr * p.hfr_factor;
        for (int yo = -1; yo < 2; yo++)
            for (int xo = -1; xo < 2; xo++) {
                const float x = sx + (float)xo * hfr;
                const float y = sy + (float)yo * hfr;
                int32_t cx = go_i32(x / g.sp_x);
                if (cx < 0) cx = 0;
                if (cx >= g.cells_x) cx = g.cells_x - 1;
                int32_t cy = go_i32(y / g.sp_y);
                if (cy < 0) cy = 0;
                if (cy >= g.cells_y) cy = g.cells_y - 1;
                std::vector<int> &c = bins[cy * g.cells_x + cx];
                if (c.empty() || !star_eq(stars[c.back()], s)) c.push_back(i);
            }
    }
    std::vector<int> star_off(ncell + 1, 0);
    for (int32_t c = 0; c < ncell; c++) star_off[c + 1] = star_off[c] + (int)bins[c].size();
    const int n_entries = star_off[ncell];
    std::vector<float> mstar(4 * (size_t)std::max(n_entries, 1), 0.0f);
    for (int32_t c = 0, e = 0; c < ncell; c++)
        for (int i : bins[c]) {
            const nl_star_t &s = stars[i];
            mstar[4 * e] = s.x;
            mstar[4 * e + 1] = s.y;
            mstar[4 * e + 2] = s.hfr * s.hfr * p.hfr_factor * p.hfr_factor;   // (:507)
            e++;
        }

    // cell rectangles (init, :146-171) and FitCell's buffer size (:147)
    const int64_t buf_size = (int64_t)go_i32(g.sp_x + 1.5f) * go_i32(g.sp_y + 1.5f);
    std::vector<int> rect(4 * (size_t)ncell);
    int max_area = 0;
    for (int32_t y = 0; y < g.cells_y; y++) {
        const int32_t y0 = go_i32((float)y * g.sp_y + 0.5f);
        int32_t y1 = go_i32(((float)y + 1) * g.sp_y + 0.5f);
        if (y1 > g.height) y1 = g.height;
        for (int32_t x = 0; x < g.cells_x; x++) {
            const int32_t x0 = go_i32((float)x * g.sp_x + 0.5f);
            int32_t x1 = go_i32(((float)x + 1) * g.sp_x + 0.5f);
            if (x1 > g.width) x1 = g.width;
            int *r = &rect[4 * (size_t)(y * g.cells_x + x)];
            r[0] = x0; r[1] = std::max(x1, x0); r[2] = y0; r[3] = std::max(y1, y0);
            max_area = std::max(max_area, (r[1] - r[0]) * (r[3] - r[2]));
        }
    }

    // device scratch
    int4 *d_rect;
    int *d_off, *d_n, *d_status, *cxl, *rbs;
    float4 *d_mstar;
    float *d_val, *dcells, *cxr, *ryr;
    auto carve = [&](void *base) {
        Carver c(base);
        d_rect = c.take<int4>(ncell);
        d_off = c.take<int>(star_off.size());
        d_mstar = c.take<float4>(mstar.size() / 4);
        d_val = c.take<float>(ncell);
        d_n = c.take<int>(ncell);
        d_status = c.take<int>(ncell);
        dcells = c.take<float>(ncell);
        cxl = c.take<int>(width);
        cxr = c.take<float>(width);
        rbs = c.take<int>(height);
        ryr = c.take<float>(height);
        return align_up(c.bytes());
    };
    NL_RUN_HIP(w.buf.reserve(carve(nullptr), stream));
    carve(w.buf.ptr);
    NL_RUN_HIP(hipMemcpyAsync(d_rect, rect.data(), sizeof(int) * rect.size(), hipMemcpyHostToDevice, stream));
    NL_RUN_HIP(hipMemcpyAsync(d_off, star_off.data(), sizeof(int) * star_off.size(), hipMemcpyHostToDevice, stream));
    NL_RUN_HIP(hipMemcpyAsync(d_mstar, mstar.data(), sizeof(float) * mstar.size(), hipMemcpyHostToDevice, stream));

    // FitCell on the device: LDS when the largest cell fits the budget, else the global staging area
    int dev = 0, lds_max = 0;
    NL_RUN_HIP(hipGetDevice(&dev));
    NL_RUN_HIP(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    const size_t sh_head = (sizeof(FitShared) + 15) & ~(size_t)15;
    const size_t lds_bytes = sh_head + sizeof(float) * (size_t)max_area;
    const bool use_lds = lds_bytes <= std::min(kLdsCap, (size_t)lds_max);
    Launcher L(stream);
    if (use_lds) {
        L(back_fit_kernel<true>, ncell, kFitThreads, lds_bytes, d_data, width, d_rect, d_off, d_mstar, p.sigma, nullptr,
          d_val, d_n, d_status);
    } else {
        NL_RUN_HIP(w.stage.reserve(sizeof(float) * (size_t)width * height, stream));
        L(back_fit_kernel<false>, ncell, kFitThreads, sh_head, d_data, width, d_rect, d_off, d_mstar, p.sigma,
          static_cast<float *>(w.stage.ptr), d_val, d_n, d_status);
    }
    NL_RUN_LAUNCHED(L);
    std::vector<float> cells(ncell);
    std::vector<int> cnt(ncell), status(ncell);
    NL_RUN_HIP(hipMemcpyAsync(cells.data(), d_val, sizeof(float) * ncell, hipMemcpyDeviceToHost, stream));
    NL_RUN_HIP(hipMemcpyAsync(cnt.data(), d_n, sizeof(int) * ncell, hipMemcpyDeviceToHost, stream));
    NL_RUN_HIP(hipMemcpyAsync(status.data(), d_status, sizeof(int) * ncell, hipMemcpyDeviceToHost, stream));
    NL_RUN_HIP(hipStreamSynchronize(stream));

    // the reference's panics in cell order; the flagged cells literally on the host
    std::vector<float> rectbuf, med, mad;
    for (int32_t c = 0; c < ncell; c++) {
        const std::string where = " in cell " + std::to_string(c % g.cells_x) + "," + std::to_string(c / g.cells_x);
        if (cnt[c] > buf_size)
            return invalid(msg, "gatherWithoutStars (background.go:511) would index past FitCell's buffer of " +
                                    std::to_string(buf_size) + " samples" + where);
        if (status[c] == kCellEmpty)
            return invalid(msg, std::string(kPanicSelect) + ": no sample left after star masking" + where);
        if (status[c] == kCellEmptyTrim)
            return invalid(msg, std::string(kPanicSelect) + ": no sample below the trimming bound" + where);
        if (status[c] != kCellHost) continue;
        const int *r = &rect[4 * (size_t)c];
        const int cw = r[1] - r[0], ch = r[3] - r[2];
        rectbuf.resize((size_t)cw * ch);
        NL_RUN_HIP(hipMemcpy2DAsync(rectbuf.data(), sizeof(float) * cw, d_data + (int64_t)r[2] * width + r[0],
                                  sizeof(float) * width, sizeof(float) * cw, ch, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipStreamSynchronize(stream));
        med.clear();
        for (int y = r[2]; y < r[3]; y++)
            for (int x = r[0]; x < r[1]; x++) {
                bool keep = true;
                for (int e = star_off[c]; e < star_off[c + 1]; e++) {
                    const float dx = (float)x - mstar[4 * e], dy = (float)y - mstar[4 * e + 1];
                    const float dist_sq = dx * dx + dy * dy;
                    if (dist_sq <= mstar[4 * e + 2]) { keep = false; break; }
                }
                if (keep) med.push_back(rectbuf[(size_t)(y - r[2]) * cw + (x - r[0])]);
            }
        const int n = (int)med.size();
        float median, madv, trimmed;
        if (!qselect_median_lit(med.data(), n, &median))
            return invalid(msg, std::string(kPanicSelect) + " (NaN pivot) selecting the median" + where);
        mad.resize(n);
        for (int i = 0; i < n; i++) mad[i] = fabsf(med[i] - median);
        if (!qselect_median_lit(mad.data(), n, &madv))
            return invalid(msg, std::string(kPanicSelect) + " (NaN pivot) selecting the MAD" + where);
        const float std_dev = madv * 1.4826f;
        const float upper_bound = median + p.sigma * std_dev;
        int kept = 0;
        for (int i = 0; i < n; i++)
            if (med[i] < upper_bound) med[kept++] = med[i];
        if (!qselect_median_lit(med.data(), kept, &trimmed))
            return invalid(msg, std::string(kPanicSelect) + (kept ? " (NaN pivot)" : ": no sample below the trimming bound") +
                                    " selecting the trimmed median" + where);
        cells[c] = trimmed;
    }

    // clip (:175-200)
    int32_t outliers = 0;
    if (p.clip > 0) {
        std::vector<float> buffer(cells);
        float threshold;
        if (!qselect_lit(buffer.data(), ncell, ncell - p.clip + 1, &threshold))
            return invalid(msg, std::string(kPanicSelect) + " (NaN pivot) selecting the clipping threshold (background.go:178)");
        for (float &cell : cells)
            if (cell >= threshold) { cell = NAN; outliers++; }
        for (int neighbors = 8; neighbors >= 0; neighbors--) {
            for (;;) {
                bool progress;
                const int changed = interpolate(cells, g.cells_x, g.cells_y, neighbors, &progress);
                if (changed == 0) break;
                if (!progress)      // (deviation 3) the same cells stay NaN on every pass: the reference loops forever
                    return invalid(msg, "clip (background.go:193-198) would loop forever: " + std::to_string(changed) +
                                            " cells stay NaN with " + std::to_string(neighbors) + " neighbours required");
            }
        }
    }

    // smoothe (:203-239) and calculateStats (:241-254)
    std::vector<float> smooth(ncell);
    for (int32_t y = 0; y < g.cells_y; y++)
        for (int32_t x = 0; x < g.cells_x; x++) {
            float sum = 0.0f, wsum = 0.0f;
            for (int32_t oy = -1; oy <= 1; oy++)
                for (int32_t ox = -1; ox <= 1; ox++) {
                    const int32_t x2 = x + ox, y2 = y + oy;
                    if (x2 >= 0 && x2 < g.cells_x && y2 >= 0 && y2 < g.cells_y) {
                        const float d = cells[x2 + y2 * g.cells_x];
                        const float wt = kGauss[ox * ox + oy * oy];
                        sum += d * wt;
                        wsum += wt;
                    }
                }
            smooth[y * g.cells_x + x] = sum / wsum;
        }
    float mn = FLT_MAX, mx = -FLT_MAX;
    for (float c : smooth) {
        if (c < mn) mn = c;
        if (c > mx) mx = c;
    }

    // Subtract's state machines and its index check (:386-462)
    std::vector<int> col_xl(width), row_yl(height);
    std::vector<float> col_xr(width), row_yr(height);
    axis_table(width, g.sp_x, g.cells_x, col_xl.data(), col_xr.data());
    axis_table(height, g.sp_y, g.cells_y, row_yl.data(), row_yr.data());
    const int64_t xl_lo = *std::min_element(col_xl.begin(), col_xl.end());
    const int64_t xl_hi = *std::max_element(col_xl.begin(), col_xl.end());
    const int64_t yl_lo = *std::min_element(row_yl.begin(), row_yl.end());
    const int64_t yl_hi = *std::max_element(row_yl.begin(), row_yl.end());
    const int64_t idx_lo = xl_lo + yl_lo * g.cells_x, idx_hi = xl_hi + yl_hi * g.cells_x + g.cells_x + 1;
    if (idx_lo < 0 || idx_hi >= ncell)
        return invalid(msg, "Subtract (background.go:445-451) would index Cells[" +
                                std::to_string(idx_lo < 0 ? idx_lo : idx_hi) + "] of a " + std::to_string(g.cells_x) +
                                "x" + std::to_string(g.cells_y) + " grid");
    std::vector<int> row_base(height);
    for (int y = 0; y < height; y++) row_base[y] = row_yl[y] * g.cells_x;

    NL_RUN_HIP(hipMemcpyAsync(dcells, smooth.data(), sizeof(float) * ncell, hipMemcpyHostToDevice, stream));
    NL_RUN_HIP(hipMemcpyAsync(cxl, col_xl.data(), sizeof(int) * width, hipMemcpyHostToDevice, stream));
    NL_RUN_HIP(hipMemcpyAsync(cxr, col_xr.data(), sizeof(float) * width, hipMemcpyHostToDevice, stream));
    NL_RUN_HIP(hipMemcpyAsync(rbs, row_base.data(), sizeof(int) * height, hipMemcpyHostToDevice, stream));
    NL_RUN_HIP(hipMemcpyAsync(ryr, row_yr.data(), sizeof(float) * height, hipMemcpyHostToDevice, stream));
    float *d_bg = nullptr;
    if (background_host) {
        NL_RUN_HIP(w.render.reserve(sizeof(float) * (size_t)width * height, stream));
        d_bg = static_cast<float *>(w.render.ptr);
    }
    const int col_blocks = (width + kSubThreads * kSubCols - 1) / (kSubThreads * kSubCols);
    const bool vec = width % kSubCols == 0 && ((uintptr_t)d_data & 15) == 0;
    with_bool(vec, [&](auto V) {
        with_bool(d_bg != nullptr, [&](auto R) {
            L(back_subtract_kernel<decltype(V)::value, decltype(R)::value>, (unsigned)col_blocks * (unsigned)height,
              kSubThreads, 0, d_data, d_bg, width, col_blocks, cxl, cxr, rbs, ryr, dcells, g.cells_x);
        });
    });
    NL_RUN_LAUNCHED(L);
    if (d_bg)
        NL_RUN_HIP(hipMemcpyAsync(background_host, d_bg, sizeof(float) * (size_t)width * height, hipMemcpyDeviceToHost,
                                stream));
    NL_RUN_HIP(hipStreamSynchronize(stream));

    if (cells_out && cells_capacity > 0)
        memcpy(cells_out, smooth.data(), sizeof(float) * (size_t)std::min<int64_t>(ncell, cells_capacity));
    if (info) {
        info->cells_x = g.cells_x;
        info->cells_y = g.cells_y;
        info->outlier_cells = outliers;
        info->spacing_x = g.sp_x;
        info->spacing_y = g.sp_y;
        info->min = mn;
        info->max = mx;
    }
    return NL_OK;
}

}  // namespace nl
