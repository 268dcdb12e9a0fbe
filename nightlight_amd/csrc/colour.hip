// colour.hip -- the rgb / lrgb command's steps around its tone curves for gfx950 (colour.hpp lists the reference lines).
//   combine_kernel       rgb.go:55-60          dest[j] = (val - min) * mult
//   rgb_clamp_kernel     pixelops.go:679-692   ScaleOffsetClampRGB, the three planes in one launch (blockIdx.y)
//   block_means_kernel   rgb.go:172-208        the per-block channel means of findDarkestBlock
//   star_sums_kernel     rgb.go:237-269        one star's disc of meanStarIntensity per lane
//   chroma_kernel        pixelops.go:448-543   pf3ChanChroma / NeutralizeBackground / ChromaForHues / RotateColors
//   export_rgb_kernel    tiff16.go:50-87, writejpg.go:48-85
// Everything is the reference's expression, operation for operation, in fp32 without FMA; sums run in the reference's
// order.  The per-pixel kernels walk their planes in quads like tone.hip (quad_common.hpp): 16-byte accesses where every
// plane they touch is 16-byte aligned, element by element where one is not.  The scalars in front of the loops and the
// short scans behind the kernels are host code below, compiled without contraction like the kernels.
#include <float.h>

#include "colour.hpp"
#include "launch_common.hpp"
#include "quad_common.hpp"

namespace nl {

namespace {

// float32(math.Max(math.Min(1, float64(x)), 0)) and float32(math.Max(0, math.Min(1, float64(x)))) alike: NaN for a
// NaN, 1 above 1, +0 for -0 and for every negative x
__device__ __forceinline__ float go_clamp01(float x)
{
    if (x != x) return x;
    if (x > 1.0f) return 1.0f;
    return x > 0.0f ? x : 0.0f;
}

struct Affine3 { float alpha[3], beta[3]; };

template <bool VEC>
__global__ __launch_bounds__(256) void combine_kernel(float *dst, const float *src, int64_t n, float min, float mult)
{
    const int64_t quads = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = load_quad<VEC>(src, q);
        store_quad<VEC>(dst, q, make_float4((v.x - min) * mult, (v.y - min) * mult, (v.z - min) * mult, (v.w - min) * mult));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (quads << 2) + threadIdx.x;
        dst[i] = (src[i] - min) * mult;
    }
}

// the clamped element 0 of every plane for the reduction's seeds (the kernel itself overwrites it)
__global__ void rgb_clamp_seed_kernel(Planes pl, Affine3 k, float *seed)
{
    const int c = threadIdx.x;
    seed[c] = go_clamp01(k.alpha[c] * pl.p[c][0] + k.beta[c]);
}

// plane blockIdx.y in place; STATS: its partials behind those of the planes before it
template <bool STATS, bool VEC>
__global__ __launch_bounds__(256) void rgb_clamp_kernel(Planes pl, int64_t n, Affine3 k, const float *seed, double *partial)
{
    const int c = blockIdx.y;
    const float alpha = k.alpha[c], beta = k.beta[c];
    quad_transform<STATS, VEC>(pl.p[c], n, [alpha, beta](float d) { return go_clamp01(alpha * d + beta); },
                               STATS ? seed + c : nullptr, STATS ? partial + 3 * (size_t)gridDim.x * c : nullptr);
}

// ---- findDarkestBlock's block means ----

constexpr int kBmTileFloats = 8192;     // 32 KiB of LDS for one chunk of a strip

// One workgroup: `nb` neighbouring blocks of one block row of one channel (blockIdx.y).  The strip goes through LDS in
// chunks of `rows` rows, loaded row by row with consecutive lanes on consecutive floats; lane (r, b) -- r fastest, the
// LDS row stride odd, so that a wave's lanes read different banks -- then sums row r of block b left to right, and lane
// b adds the chunk's row sums to its block's sum top to bottom.  rows * nb <= 256.  STAGED false: the same without the
// LDS, every row taken from global memory (blocks of more than kBmTileFloats - 1 columns, and the developer switch).
struct BmGeom {
    int width, x_first, y_first, nbx, groups;   // groups: workgroups per block row
    int block, nb, ld, rows;
    float inv;
};

template <bool STAGED>
__global__ __launch_bounds__(256) void block_means_kernel(Planes pl, BmGeom g, float *means)
{
    __shared__ float tile[STAGED ? kBmTileFloats : 1];
    __shared__ float row_sum[256];
    const float *src = pl.p[blockIdx.y];
    const int tid = threadIdx.x;
    const int by = blockIdx.x / g.groups, b0 = (blockIdx.x - by * g.groups) * g.nb;
    const int nb = min(g.nb, g.nbx - b0);
    const int x0 = g.x_first + b0 * g.block, y0 = g.y_first + by * g.block, tw = nb * g.block;
    const int b = tid / g.rows, r = tid - b * g.rows;
    float acc = 0.0f;
    for (int c0 = 0; c0 < g.block; c0 += g.rows) {
        const int rc = min(g.rows, g.block - c0);
        if constexpr (STAGED) {
            for (int rr = 0; rr < rc; rr++) {
                const float *row = src + (int64_t)(y0 + c0 + rr) * g.width + x0;
                for (int cc = tid; cc < tw; cc += 256) tile[rr * g.ld + cc] = row[cc];
            }
            __syncthreads();
        }
        if (r < rc && b < nb) {
            const float *row = STAGED ? tile + r * g.ld + b * g.block
                                      : src + (int64_t)(y0 + c0 + r) * g.width + x0 + b * g.block;
            float s = 0.0f;                                              // rowSum := float32(0)
            for (int i = 0; i < g.block; i++) s += row[i];
            row_sum[b * g.rows + r] = s;
        }
        __syncthreads();
        if (tid < nb)
            for (int rr = 0; rr < rc; rr++) acc += row_sum[tid * g.rows + rr];
        __syncthreads();
    }
    if (tid < nb) means[((int64_t)by * g.nbx + b0 + tid) * 3 + blockIdx.y] = acc * g.inv;
}

// ---- meanStarIntensity: one star per lane ----

__global__ __launch_bounds__(64) void star_sums_kernel(Planes pl, int width, int height, const nl_star_t *stars, int n,
                                                       nl_rgb_t clip, StarSum *out)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const nl_star_t s = stars[i];
    const int32_t star_x = s.index % width, star_y = s.index / width;   // (truncation, as Go)
    const float hfr = s.hfr * 0.75f;
    const int32_t hfr_r = go_i32(hfr + 0.5f);
    const float t = hfr + 0.01f;
    const float hfr_sq = t * t;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
    int32_t pixels = 0;
    for (int32_t off_y = -hfr_r; off_y <= hfr_r; off_y++) {
        const int32_t y = star_y + off_y;
        if (y < 0 || y >= height) continue;
        for (int32_t off_x = -hfr_r; off_x <= hfr_r; off_x++) {
            const int32_t x = star_x + off_x;
            if (x < 0 || x >= width) continue;
            const float dist_sq = (float)(off_x * off_x + off_y * off_y);
            if (dist_sq <= hfr_sq) {
                const int32_t at = y * width + x;
                const float r = pl.p[0][at], g = pl.p[1][at], b = pl.p[2][at];
                if (r < clip.r && g < clip.g && b < clip.b) {
                    sr += r;
                    sg += g;
                    sb += b;
                    pixels++;
                }
            }
        }
    }
    out[i] = StarSum{sr, sg, sb, pixels};
}

// ---- the chroma and hue steps: the target plane's new value from the deciding plane's and its own ----

struct ChromaArgs { float a, b, c, d; double gg; };

// pixelops.go:504-505 / :537-538, as written: strict, wrapping when from > to; a NaN hue fails every compare
__device__ __forceinline__ bool hue_in_range(float h, float from, float to)
{
    return (from <= to && (h > from && h < to)) || (from > to && (h > from || h < to));
}

template <int KIND>
__device__ __forceinline__ float chroma_pixel(float decide, float target, const ChromaArgs &p)
{
    if constexpr (KIND == NL_CHROMA_GAMMA) {                 // decide l, target c; a = threshold
        if (decide < p.a) return target;                     // :452 (a NaN luminance goes on to the power)
        return pow_f32(target, p.gg);                        // :453
    } else if constexpr (KIND == NL_CHROMA_NEUTRALIZE) {     // decide l, target c; a = low (= high, :473)
        return decide < p.a ? 0.0f : target;                 // :477-478; :479 never holds
    } else if constexpr (KIND == NL_CHROMA_FOR_HUES) {       // decide h, target c; a, b, c = from, to, factor
        return hue_in_range(decide, p.a, p.b) ? go_clamp01(target * p.c) : target;      // :504-508
    } else {                                                 // decide l, target h; a, b, c, d = from, to, offset, lthres
        if (decide < p.d) return target;                     // :533
        return hue_in_range(target, p.a, p.b) ? target + p.c : target;                  // :537-540
    }
}

// a pixel the reference leaves alone is stored back with the bits it had
template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void chroma_kernel(const float *decide, float *target, int64_t n, ChromaArgs p)
{
    const int64_t quads = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 d = load_quad<VEC>(decide, q), t = load_quad<VEC>(target, q);
        store_quad<VEC>(target, q, make_float4(chroma_pixel<KIND>(d.x, t.x, p), chroma_pixel<KIND>(d.y, t.y, p),
                                               chroma_pixel<KIND>(d.z, t.z, p), chroma_pixel<KIND>(d.w, t.w, p)));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (quads << 2) + threadIdx.x;
        target[i] = chroma_pixel<KIND>(decide[i], target[i], p);
    }
}

// ---- the colour export: four pixels per lane ----

// high byte first
__device__ __forceinline__ unsigned be16(unsigned c) { return (c >> 8) | ((c & 255u) << 8); }

// one pixel's R G B A: two little-endian words of four big-endian uint16 (image.RGBA64.Pix), or one word of four bytes
// (image.RGBA.Pix)
template <int BITS, bool GAMMA>
__device__ __forceinline__ uint2 rgba_words(float r, float g, float b, float min, float scale, double gamma_inv)
{
    const unsigned cr = gray_count<BITS, GAMMA>(r, min, scale, gamma_inv);
    const unsigned cg = gray_count<BITS, GAMMA>(g, min, scale, gamma_inv);
    const unsigned cb = gray_count<BITS, GAMMA>(b, min, scale, gamma_inv);
    if constexpr (BITS == 16) return make_uint2(be16(cr) | (be16(cg) << 16), be16(cb) | 0xffff0000u);
    else return make_uint2(cr | (cg << 8) | (cb << 16) | 0xff000000u, 0u);
}

template <int BITS, bool GAMMA, bool VEC>
__global__ __launch_bounds__(256) void export_rgb_kernel(Planes pl, int64_t n, float min, float scale, double gamma_inv,
                                                         unsigned char *out)
{
    const int64_t quads = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 r = load_quad<VEC>(pl.p[0], q), g = load_quad<VEC>(pl.p[1], q), b = load_quad<VEC>(pl.p[2], q);
        const uint2 w0 = rgba_words<BITS, GAMMA>(r.x, g.x, b.x, min, scale, gamma_inv);
        const uint2 w1 = rgba_words<BITS, GAMMA>(r.y, g.y, b.y, min, scale, gamma_inv);
        const uint2 w2 = rgba_words<BITS, GAMMA>(r.z, g.z, b.z, min, scale, gamma_inv);
        const uint2 w3 = rgba_words<BITS, GAMMA>(r.w, g.w, b.w, min, scale, gamma_inv);
        uint4 *o = reinterpret_cast<uint4 *>(out);
        if constexpr (BITS == 16) {
            o[2 * q] = make_uint4(w0.x, w0.y, w1.x, w1.y);
            o[2 * q + 1] = make_uint4(w2.x, w2.y, w3.x, w3.y);
        } else {
            o[q] = make_uint4(w0.x, w1.x, w2.x, w3.x);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (quads << 2) + threadIdx.x;
        const uint2 w = rgba_words<BITS, GAMMA>(pl.p[0][i], pl.p[1][i], pl.p[2][i], min, scale, gamma_inv);
        if constexpr (BITS == 16) reinterpret_cast<uint2 *>(out)[i] = w;
        else reinterpret_cast<unsigned *>(out)[i] = w.x;
    }
}

bool planes_ok(const Planes &pl)
{
    return pl.p[0] && pl.p[1] && pl.p[2];
}

bool planes_aligned16(const Planes &pl)
{
    return aligned16(pl.p[0]) && aligned16(pl.p[1]) && aligned16(pl.p[2]);
}

// Go's float32 -> int (64 bits) is CVTTSS2SQ on amd64: truncation, 0x8000000000000000 for NaN or out of range
int64_t go_i64(float f)
{
    return (f >= -9223372036854775808.0f && f < 9223372036854775808.0f) ? (int64_t)f : INT64_MIN;
}

}  // namespace

// ---- host scalars ----

void rgb_normalization(const float mins[3], const float maxs[3], float *min, float *mult)
{
    float lo = mins[0], hi = maxs[0];
    for (int c = 1; c < 3; c++) {
        if (mins[c] < lo) lo = mins[c];
        if (maxs[c] > hi) hi = maxs[c];
    }
    *min = lo;
    *mult = 1.0f / (hi - lo);
}

void rgb_balance_coeffs(nl_rgb_t cs, nl_rgb_t ch, nl_rgb_t ts, nl_rgb_t th, float alpha[3], float beta[3])
{
    const float new_shadow = (cs.r + cs.g + cs.b) / 3.0f;                                   // rgb.go:127
    const float ns[3] = {ts.r * new_shadow, ts.g * new_shadow, ts.b * new_shadow};
    const float new_highlight = (ch.r + ch.g + ch.b) / 3.0f;                                // :132
    const float nh[3] = {th.r * new_highlight, th.g * new_highlight, th.b * new_highlight};
    const float cur_s[3] = {cs.r, cs.g, cs.b}, cur_h[3] = {ch.r, ch.g, ch.b};
    for (int c = 0; c < 3; c++) {
        alpha[c] = (nh[c] - ns[c]) / (cur_h[c] - cur_s[c]);                                 // :137-139
        beta[c] = ns[c] - alpha[c] * cur_s[c];                                              // :142-144
    }
}

BlockGrid darkest_block_grid(int width, int height, int block, float border)
{
    BlockGrid g;
    g.x_first = (go_i32((float)width * border) / block) * block;                            // rgb.go:158-162
    g.x_last = ((width - g.x_first) / block) * block;
    g.y_first = (go_i32((float)height * border) / block) * block;
    g.y_last = ((height - g.y_first) / block) * block;
    g.inv_block_pixels = 1.0f / (float)(int32_t)((uint32_t)block * (uint32_t)block);        // :163 (int32, wrapping)
    g.nbx = g.x_last > g.x_first ? (g.x_last - g.x_first) / block : 0;
    g.nby = g.y_last > g.y_first ? (g.y_last - g.y_first) / block : 0;
    return g;
}

nl_rgb_t darkest_block_scan(const float *means, int64_t n_blocks)
{
    float r_min = FLT_MAX, g_min = FLT_MAX, b_min = FLT_MAX, l_min = FLT_MAX;               // rgb.go:165-169
    for (int64_t i = 0; i < n_blocks; i++) {
        const float r = means[3 * i], g = means[3 * i + 1], b = means[3 * i + 2];
        const float l = (r + g + b) / 3.0f;                                                 // :211
        if (l < l_min) { r_min = r; g_min = g; b_min = b; l_min = l; }
    }
    return nl_rgb_t{r_min, g_min, b_min};
}

void star_range(int n_stars, float skip_bright, float skip_dim, int64_t *s_start, int64_t *s_end)
{
    *s_start = go_i64((float)n_stars * skip_bright);                                        // rgb.go:226-227
    *s_end = (int64_t)((uint64_t)(int64_t)n_stars - (uint64_t)go_i64((float)n_stars * skip_dim));
}

int32_t star_hfr_radius(float hfr_field)
{
    const float hfr = hfr_field * 0.75f;
    return go_i32(hfr + 0.5f);
}

nl_rgb_t star_mean(const StarSum *sums, int n)
{
    float tr = 0.0f, tg = 0.0f, tb = 0.0f;
    int32_t pixels = 0;
    for (int i = 0; i < n; i++) {                                                           // rgb.go:272-275
        tr += sums[i].r;
        tg += sums[i].g;
        tb += sums[i].b;
        pixels = (int32_t)((uint32_t)pixels + (uint32_t)sums[i].pixels);
    }
    const float norm = 1.0f / (float)pixels;                                                // :279 (0 pixels: 0 * +Inf)
    return nl_rgb_t{tr * norm, tg * norm, tb * norm};
}

// ---- launchers ----

hipError_t launch_combine(float *d_dst, const float *d_src, int64_t n, float min, float mult, hipStream_t stream)
{
    if (n < 1 || !d_dst || !d_src) return hipErrorInvalidValue;
    Launcher L(stream);
    with_bool(aligned16(d_dst) && aligned16(d_src), [&](auto V) {
        L(combine_kernel<decltype(V)::value>, quad_blocks(n), 256, 0, d_dst, d_src, n, min, mult);
    });
    return L.err;
}

hipError_t launch_rgb_clamp(Planes planes, int64_t n, const float alpha[3], const float beta[3], float *seed,
                            double *partial, int blocks, hipStream_t stream)
{
    if (n < 1 || !planes_ok(planes) || (partial && (!seed || blocks < 1))) return hipErrorInvalidValue;
    const Affine3 k{{alpha[0], alpha[1], alpha[2]}, {beta[0], beta[1], beta[2]}};
    Launcher L(stream);
    with_bool(planes_aligned16(planes), [&](auto V) {
        constexpr bool vec = decltype(V)::value;
        if (partial) {
            L(rgb_clamp_seed_kernel, 1, 3, 0, planes, k, seed);
            L(rgb_clamp_kernel<true, vec>, dim3(blocks, 3), 256, 0, planes, n, k, seed, partial);
        } else {
            L(rgb_clamp_kernel<false, vec>, dim3(quad_blocks(n), 3), 256, 0, planes, n, k, nullptr, nullptr);
        }
    });
    return L.err;
}

hipError_t launch_block_means(Planes planes, int width, const BlockGrid &grid, int block, bool direct, float *d_means,
                              hipStream_t stream)
{
    if (!planes_ok(planes) || !d_means || block < 1 || grid.nbx < 1 || grid.nby < 1) return hipErrorInvalidValue;
    BmGeom g;
    g.width = width;
    g.x_first = grid.x_first;
    g.y_first = grid.y_first;
    g.nbx = grid.nbx;
    g.block = block;
    g.inv = grid.inv_block_pixels;
    g.nb = std::min(grid.nbx, std::max(1, 256 / block));
    g.ld = (int)(((int64_t)g.nb * block) | 1);
    const bool staged = !direct && (int64_t)g.nb * block < kBmTileFloats;
    g.rows = std::min(block, 256 / g.nb);
    if (staged) g.rows = std::min(g.rows, kBmTileFloats / g.ld);
    g.groups = (grid.nbx + g.nb - 1) / g.nb;
    const int64_t wgs = (int64_t)g.groups * grid.nby;
    if (wgs > 0x7fffffff) return hipErrorInvalidValue;
    Launcher L(stream);
    with_bool(staged, [&](auto S) {
        L(block_means_kernel<decltype(S)::value>, dim3((unsigned)wgs, 3), 256, 0, planes, g, d_means);
    });
    return L.err;
}

hipError_t launch_star_sums(Planes planes, int width, int height, const nl_star_t *d_stars, int n, nl_rgb_t clip,
                            StarSum *d_sums, hipStream_t stream)
{
    if (!planes_ok(planes) || !d_stars || !d_sums || n < 1) return hipErrorInvalidValue;
    Launcher L(stream);
    L(star_sums_kernel, (n + 63) / 64, 64, 0, planes, width, height, d_stars, n, clip, d_sums);
    return L.err;
}

bool chroma_kind_known(int kind)
{
    return kind >= NL_CHROMA_GAMMA && kind <= NL_ROTATE_HUES;
}

hipError_t launch_chroma(Planes planes, int64_t n, const nl_chroma_t &op, hipStream_t stream)
{
    if (n < 1 || !planes_ok(planes) || !chroma_kind_known(op.kind)) return hipErrorInvalidValue;
    const float *h = planes.p[0], *l = planes.p[2];
    float *hue = planes.p[0], *c = planes.p[1];
    Launcher L(stream);
    auto run = [&](auto KIND, const float *decide, float *target, ChromaArgs a) {
        with_bool(aligned16(decide) && aligned16(target), [&](auto V) {
            L(chroma_kernel<decltype(KIND)::value, decltype(V)::value>, quad_blocks(n), 256, 0, decide, target, n, a);
        });
    };
    switch (op.kind) {
    case NL_CHROMA_GAMMA:                      // p = {gamma, threshold}; gg := float64(1.0 / gamma), pixelops.go:450
        run(std::integral_constant<int, NL_CHROMA_GAMMA>{}, l, c, ChromaArgs{op.p[1], 0.0f, 0.0f, 0.0f, (double)(1.0f / op.p[0])});
        break;
    case NL_CHROMA_NEUTRALIZE:                 // p = {low, high}; high is never read (:473)
        run(std::integral_constant<int, NL_CHROMA_NEUTRALIZE>{}, l, c, ChromaArgs{op.p[0], 0.0f, 0.0f, 0.0f, 0.0});
        break;
    case NL_CHROMA_FOR_HUES:                   // p = {from, to, factor}
        run(std::integral_constant<int, NL_CHROMA_FOR_HUES>{}, h, c, ChromaArgs{op.p[0], op.p[1], op.p[2], 0.0f, 0.0});
        break;
    default:                                   // NL_ROTATE_HUES, p = {from, to, offset, lthres}
        run(std::integral_constant<int, NL_ROTATE_HUES>{}, l, hue, ChromaArgs{op.p[0], op.p[1], op.p[2], op.p[3], 0.0});
        break;
    }
    return L.err;
}

hipError_t launch_export_rgb(Planes planes, int64_t n, float min, float scale, bool use_gamma, double gamma_inv, int bits,
                             void *d_out, hipStream_t stream)
{
    if (n < 1 || !planes_ok(planes) || !d_out || !aligned16(d_out) || (bits != 8 && bits != 16)) return hipErrorInvalidValue;
    Launcher L(stream);
    with_bool(bits == 16, [&](auto WIDE) {
        with_bool(use_gamma, [&](auto G) {
            with_bool(planes_aligned16(planes), [&](auto V) {
                L(export_rgb_kernel<decltype(WIDE)::value ? 16 : 8, decltype(G)::value, decltype(V)::value>,
                  quad_blocks(n), 256, 0, planes, n, min, scale, gamma_inv, static_cast<unsigned char *>(d_out));
            });
        });
    });
    return L.err;
}

}  // namespace nl
