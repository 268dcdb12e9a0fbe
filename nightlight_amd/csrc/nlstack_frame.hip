// nlstack_frame.hip -- steps on one resident frame that belong to no single command: statistics, location and scale,
// and noise (stats.go, noise.go; the estimators' kernels in locscale.hip), the affine step, the median filters (ops/pre/badpixels.go:54-77, internal/median/gather.go:26-38), OpAlign's
// projection from a resident frame, and what the four units of the frame steps share (nlstack_frame_common.hpp; the
// others: nlstack_frame_pre.hip, _stretch.hip, _rgb.hip).  Kernels in frame_stats.hip and project.hip.
#include <assert.h>
#include <math.h>

#include <algorithm>

#include "bayer.hpp"
#include "nlstack_frame_common.hpp"

namespace {

// one whole frame through a filter kernel, launch(d_in, d_out), on `device`: buffers of its own, no handle
template <class Launch>
int median_filter_run(const char *who, const float *in_host, float *out_host, int64_t n, int device, Launch launch)
{
    int rc = select_device(device);
    if (rc != NL_OK) return rc;
    const size_t bytes = (size_t)n * sizeof(float);
    float *d_in = nullptr, *d_out = nullptr;
    NL_HIP(dev_malloc(&d_in, bytes));
    hipError_t e = dev_malloc(&d_out, bytes);
    if (e != hipSuccess) { (void)hipFree(d_in); return fail(NL_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
    do {
        if ((e = hipMemcpy(d_in, in_host, bytes, hipMemcpyHostToDevice)) != hipSuccess) break;
        if ((e = launch(d_in, d_out)) != hipSuccess) break;
        if ((e = hipMemcpy(out_host, d_out, bytes, hipMemcpyDeviceToHost)) != hipSuccess) break;
    } while (0);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(NL_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    return NL_OK;
}

// the checks both forms share; *s = the source slot, *d = the destination slot, inv = the inverse transform
int project_from_check(const char *who, nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float *trans,
                       float **s, float **d, float inv[6])
{
    char src_part[96], dst_part[96];
    snprintf(src_part, sizeof src_part, "%s (source)", who);
    snprintf(dst_part, sizeof dst_part, "%s (destination)", who);
    int rc = resident_target(src, src_idx, src_part, false, s);
    if (rc == NL_OK) rc = resident_target(dst, dst_idx, dst_part, false, d);
    if (rc != NL_OK) return rc;
    if (!trans) return fail(NL_ERR_INVALID_ARG, "%s: null transform", who);
    rc = need_whole_image(src, src_part, "a projection reads any row of the source");
    if (rc == NL_OK) rc = need_int32_pixels(src->npix, who, "source frame");
    if (rc == NL_OK) rc = need_int32_pixels(dst->npix, who, "destination tile");
    if (rc != NL_OK) return rc;
    if (dst->d_frames != dst->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "%s: the destination's frames are attached, not owned", who);
    if (*s == *d) return fail(NL_ERR_INVALID_ARG, "%s: slot %d of one handle is source and destination (a projection cannot run in place)", who, src_idx);
    return invert_transform(trans, inv);
}

// the source rows [*y0, *y1] that the destination rows of dst can tap (project.hpp: the corners of a rectangle bound
// every pixel's coordinates) with a kernel of radius grow + 1; false: none
bool project_source_rows(const nl_stack_t *dst, const nl_stack_t *src, const float inv[6], int grow, int *y0, int *y1)
{
    const nl::ProjInv t = {inv[0], inv[1], inv[2], inv[3], inv[4], inv[5]};
    const float px[2] = {0.0f, (float)(dst->width - 1)}, py[2] = {(float)dst->row0, (float)(dst->row0 + dst->rows - 1)};
    float lo = INFINITY, hi = -INFINITY;
    for (int i = 0; i < 4; i++) {
        const float y = nl::proj_y(t, px[i & 1], py[i >> 1]);
        if (y != y || !isfinite(inv[3]) || !isfinite(inv[4]) || !isfinite(inv[5])) { lo = -INFINITY; hi = INFINITY; break; }
        lo = fminf(lo, y);
        hi = fmaxf(hi, y);
    }
    *y0 = std::max(nl::proj_floor_clamped(lo) - grow, 0);
    *y1 = std::min(nl::proj_floor_clamped(hi) + 1 + grow, src->height - 1);
    return *y0 <= *y1;
}

}  // namespace

// ---- what the four units share (nlstack_frame_common.hpp) ---------------------------------------------------------

int nl::resident_target(nl_stack_t *h, int idx, const char *who, bool result_ok, float **d)
{
    if (idx < 0 && result_ok) {
        if (h->last_mode < 0) return fail(NL_ERR_INVALID_ARG, "%s: the handle has not run a pass", who);
        *d = h->d_out;
        return NL_OK;
    }
    if (idx >= 0) NL_SETTLE_UPLOADS(h);
    if (idx < 0 || idx >= h->n_frames) return fail(NL_ERR_INVALID_ARG, "%s: bad index %d", who, idx);
    *d = h->d_frames + (int64_t)idx * h->fstride;
    return NL_OK;
}

int nl::resident_entry(nl_stack_t *h, int idx, const char *who, bool result_ok, float **d)
{
    NL_CHECK_HANDLE(h);
    return resident_target(h, idx, who, result_ok, d);
}

int nl::need_whole_image(const nl_stack_t *h, const char *who, const char *why)
{
    if (h->row0 == 0 && h->rows == h->height) return NL_OK;
    return fail(NL_ERR_INVALID_ARG, "%s needs a whole-image handle (%s)", who, why);
}

int nl::need_int32_pixels(int64_t n, const char *who, const char *what)
{
    if (n < ((int64_t)1 << 31)) return NL_OK;
    return fail(NL_ERR_INVALID_ARG, "%s: %s of 2^31 pixels or more", who, what);
}

int nl::need_whole_frame(const nl_stack_t *h, const char *who, const char *why)
{
    const int rc = need_whole_image(h, who, why);
    return rc == NL_OK ? need_int32_pixels(h->npix, who) : rc;
}

// getOffsets (debayer.go:26-37)
int nl::cfa_offsets(const char *cfa, int *xo, int *yo)
{
    const std::string c = cfa;
    if (c == "RGGB" || c == "rggb") { *xo = 0; *yo = 0; }
    else if (c == "GRBG" || c == "grbg") { *xo = 1; *yo = 0; }
    else if (c == "GBRG" || c == "gbrg") { *xo = 0; *yo = 1; }
    else if (c == "BGGR" || c == "bggr") { *xo = 1; *yo = 1; }
    else return fail(NL_ERR_INVALID_ARG, "Unknown CFA value %s", cfa);
    return NL_OK;
}

int nl::cfa_names(const char *channel, const char *cfa, int *ch, int *xo, int *yo)
{
    if (const int rc = cfa_offsets(cfa, xo, yo); rc != NL_OK) return rc;
    // the channel switch of CosmeticCorrectionBayer / DebayerBilinear (badpixels_bayer.go:36-45, debayer.go:47-59)
    const std::string c = channel;
    if (c == "R" || c == "r") *ch = nl::kBayerR;
    else if (c == "G" || c == "g") *ch = nl::kBayerG;
    else if (c == "B" || c == "b") *ch = nl::kBayerB;
    else return fail(NL_ERR_INVALID_ARG, "Unknown debayering value %s", channel);
    return NL_OK;
}

int nl::check_capacity(const char *who, int capacity, const void *ptr)
{
    if (capacity < 0 || (capacity > 0 && !ptr))
        return fail(NL_ERR_INVALID_ARG, "%s: capacity %d with %s output", who, capacity, ptr ? "an" : "no");
    return NL_OK;
}

int nl::check_stars(const char *who, const nl_star_t *stars, int n_stars)
{
    if (n_stars < 0 || (n_stars > 0 && !stars)) return fail(NL_ERR_INVALID_ARG, "%s: %d stars", who, n_stars);
    return NL_OK;
}

int nl::export_check(const char *who, float gamma, int bits, const void *out_host)
{
    if (!out_host) return fail(NL_ERR_INVALID_ARG, "%s: null output", who);
    if (bits != 8 && bits != 16) return fail(NL_ERR_INVALID_ARG, "%s: %d bits (8: image.Gray, 16: image.Gray16)", who, bits);
    if (!(gamma > 0.0f))                       // (deviation: gray becomes infinite or NaN in front of the conversion)
        return fail(NL_ERR_INVALID_ARG, "%s: gamma %g (tiff16.go:113, writejpg.go:111: a positive number)", who, gamma);
    return NL_OK;
}

int nl::export_impl(nl_stack_t *h, const float *gray, const Planes *rgb, float min, float max, float gamma, int bits,
                    void *out_host)
{
    const float scale = 1.0f / (max - min);                    // tiff16.go:50-51, :112-113
    const double ginv = (double)(1.0f / gamma);
    const size_t bytes = (size_t)h->npix * (size_t)(rgb ? bits / 2 : bits / 8);
    NL_HIP(h->ingest.reserve(bytes, h->stream));
    NL_HIP(rgb ? launch_export_rgb(*rgb, h->npix, min, scale, ginv != 1.0, ginv, bits, h->ingest.ptr, h->stream)
               : launch_export_gray(gray, h->npix, min, scale, ginv != 1.0, ginv, bits, h->ingest.ptr, h->stream));
    NL_HIP(hipMemcpyAsync(out_host, h->ingest.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl::sum_stat_partials(nl_stack_t *h, double *sum)
{
    std::vector<double> part(kStatBlocks);
    NL_HIP(hipMemcpyAsync(part.data(), h->d_stat_partial, sizeof(double) * kStatBlocks,
                          hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (int b = 0; b < kStatBlocks; b++) s += part[b];
    *sum = s;
    return NL_OK;
}

nl::MinSumMax nl::fold_min_sum_max(const std::vector<double> &part)
{
    MinSumMax f{(float)part[0], 0.0, (float)part[2]};
    for (int b = 0; b < kStatBlocks; b++) {
        const float bl = (float)part[3 * b], bh = (float)part[3 * b + 2];
        if (bl < f.lo) f.lo = bl;
        if (bh > f.hi) f.hi = bh;
        f.sum += part[3 * b + 1];
    }
    return f;
}

int nl::min_mean_max_from_partials(nl_stack_t *h, int64_t n, float *mn, float *mean, float *mx, const double *d_part)
{
    std::vector<double> part(3 * kStatBlocks);
    NL_HIP(hipMemcpyAsync(part.data(), d_part ? d_part : h->d_stat_partial, sizeof(double) * 3 * kStatBlocks,
                          hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    const MinSumMax f = fold_min_sum_max(part);
    if (mn) *mn = f.lo;
    if (mx) *mx = f.hi;
    if (mean) *mean = (float)(f.sum / (double)n);
    return NL_OK;
}

int nl::frame_stats_impl(nl_stack_t *h, const float *d, int64_t n, float *mn, float *mean, float *mx, double *variance)
{
    float m = 0.0f;
    NL_HIP(nl::launch_min_sum_max(d, n, h->d_stat_partial, kStatBlocks, h->stream));
    int rc = min_mean_max_from_partials(h, n, mn, &m, mx);
    if (rc != NL_OK) return rc;
    if (mean) *mean = m;
    if (variance) {
        NL_HIP(nl::launch_variance(d, n, m, h->d_stat_partial, kStatBlocks, h->stream));
        double s;
        if ((rc = sum_stat_partials(h, &s)) != NL_OK) return rc;
        *variance = s / (double)n;
    }
    return NL_OK;
}

// everything enqueued on the handle so far has finished (the group settles the source once, before its tiles' threads)
int nl::stack_settle(nl_stack_t *h)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// Both C-ABI forms.  The group's (from_group): the source is settled and is only read here, since the tiles run on
// threads of their own; a destination on another device than the source first receives the source rows it can tap,
// peer to peer, at their place in its ingest buffer.
int nl::stack_project_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float trans[6],
                           float out_of_bounds, const char *who, bool from_group, int kernel, int clamp)
{
    NL_CHECK_HANDLE(src);
    NL_CHECK_HANDLE(dst);
    if (src->device != dst->device && !from_group)
        return fail(NL_ERR_INVALID_ARG, "%s: source on device %d, destination on device %d", who, src->device, dst->device);
    assert(!from_group || !src->uploads_pending);               // (nl::stack_settle: the tiles' threads only read src)
    float *s = nullptr, *d = nullptr;
    float inv[6];
    int rc = project_from_check(who, dst, dst_idx, src, src_idx, trans, &s, &d, inv);
    if (rc != NL_OK) return rc;
    if (src != dst && !from_group && (rc = nl_stack_order_stream_after(src, dst->stream)) != NL_OK) return rc;
    NL_HIP(hipSetDevice(dst->device));
    if (src->device != dst->device) {
        NL_HIP(dst->ingest.reserve((size_t)src->npix * sizeof(float), dst->stream));
        int y0 = 0, y1 = 0;
        if (project_source_rows(dst, src, inv, kernel, &y0, &y1)) {               // (NL_RS_*: the radius - 1)
            const size_t at = (size_t)y0 * (size_t)src->width;
            NL_HIP(hipMemcpyPeerAsync(static_cast<float *>(dst->ingest.ptr) + at, dst->device, s + at, src->device,
                                      sizeof(float) * (size_t)(y1 - y0 + 1) * (size_t)src->width, dst->stream));
        }
        s = static_cast<float *>(dst->ingest.ptr);
    }
    if (kernel == NL_RS_BILINEAR) {
        NL_HIP(nl::launch_project_tiled(s, src->width, src->height, d, dst->width, dst->row0, dst->rows, inv, out_of_bounds,
                                        project_switches(dst), dst->stream));
    } else {                                                   // include/nlstack_resample.h (an extension)
        const float *table = nullptr;
        if (kernel == NL_RS_LANCZOS3) NL_HIP(nl::lanczos3_table_device(dst->device, &table));
        NL_HIP(nl::launch_resample_tiled(s, src->width, src->height, d, dst->width, dst->row0, dst->rows, inv, out_of_bounds,
                                         kernel + 1, clamp != 0, table, project_switches(dst), dst->stream));
    }
    NL_HIP(hipStreamSynchronize(dst->stream));                 // the caller may overwrite the source slot at once
    return NL_OK;
}

int nl::resample_args_check(const char *who, int kernel, const float *trans)
{
    if (kernel != NL_RS_BILINEAR && kernel != NL_RS_BICUBIC && kernel != NL_RS_LANCZOS3)
        return fail(NL_ERR_INVALID_ARG, "%s: unknown kernel %d (NL_RS_BILINEAR 0, NL_RS_BICUBIC 1, NL_RS_LANCZOS3 2)", who, kernel);
    if (!trans) return fail(NL_ERR_INVALID_ARG, "%s: null transform", who);
    float inv[6];
    return invert_transform(trans, inv);
}

extern "C" {

// ---- per-frame statistics ---------------------------------------------------

int nl_stack_frame_stats(nl_stack_t *h, int idx, float *mn, float *mean, float *mx, double *variance)
{
    float *d;
    const int rc = resident_entry(h, idx, "frame_stats", false, &d);
    return rc == NL_OK ? frame_stats_impl(h, d, h->npix, mn, mean, mx, variance) : rc;
}

// ---- Stats.Location() / Scale() (stats.go:225-244; kernels and the sampling calls in locscale.hip) ----------------

// what needs no device: the estimator, the sample count, the seeds it reads
static int locscale_check(const char *who, int estimator, int num_samples, const uint32_t *seeds, int n_seeds,
                          float *location, float *scale)
{
    if (!location || !scale) return fail(NL_ERR_INVALID_ARG, "%s: null output", who);
    if (estimator == NL_LSE_IKSS)
        return fail(NL_ERR_INVALID_ARG, "%s: estimator %d, LSEIKSS (stats.go:535-566), sorts the whole frame: not implemented on the device",
                    who, estimator);
    if (estimator < NL_LSE_MEAN_STDDEV || estimator > NL_LSE_HISTOGRAM)
        return fail(NL_ERR_INVALID_ARG, "%s: unknown estimator %d (stats.go:31-37)", who, estimator);
    const int need = estimator == NL_LSE_MEDIAN_MAD ? 2 : estimator == NL_LSE_SC_MEDIAN_QN ? NL_LOCSCALE_MAX_SEEDS : 0;
    if (need == 0) return NL_OK;
    if (num_samples < 4 || num_samples > nl::kLocScaleMaxSamples)
        return fail(NL_ERR_INVALID_ARG, "%s: %d samples (4 .. %d)", who, num_samples, nl::kLocScaleMaxSamples);
    if (n_seeds < need || !seeds)
        return fail(NL_ERR_INVALID_ARG, "%s: %d seeds, estimator %d reads %d", who, seeds ? n_seeds : 0, estimator, need);
    for (int i = 0; i < need; i++)
        if (seeds[i] == 0)
            return fail(NL_ERR_INVALID_ARG, "%s: seed %d is zero (fastrand would replace it by one from the clock)", who, i);
    return NL_OK;
}

static int locscale_impl(nl_stack_t *h, const float *d, const char *who, int estimator, int num_samples,
                         const uint32_t *seeds, const float *min_max, float *location, float *scale,
                         nl_locscale_t *info)
{
    int rc = need_whole_frame(h, who, "the samples come from the whole frame");
    if (rc != NL_OK) return rc;
    if (h->npix < 2) return fail(NL_ERR_INVALID_ARG, "%s: a frame of %lld pixels (Uint32n(len(data) - 1), stats.go:440)", who, (long long)h->npix);
    nl_locscale_t out{};
    if (estimator == NL_LSE_MEAN_STDDEV) {                      // :229-230, StdDev() :134-144
        double variance;
        if ((rc = frame_stats_impl(h, d, h->npix, &out.min, location, &out.max, &variance)) != NL_OK) return rc;
        *scale = (float)sqrt(variance);
    } else {
        if (estimator == NL_LSE_MEDIAN_MAD) ;                  // (reads neither Min() nor Max(): info keeps 0, 0)
        else if (min_max) { out.min = min_max[0]; out.max = min_max[1]; }
        else if ((rc = frame_stats_impl(h, d, h->npix, &out.min, nullptr, &out.max, nullptr)) != NL_OK) return rc;
        if (estimator == NL_LSE_SC_MEDIAN_QN) out.epsilon = (out.max - out.min) / 65535.0f;       // :239
        std::string msg;
        rc = nl::locscale_run(d, h->npix, estimator, num_samples, seeds, out.min, out.max, h->frame_scratch.locscale_work,
                              h->stream, location, scale, &out, &msg);
        if (rc != NL_OK) fail(rc, "%s: %s", who, msg.c_str());
    }
    if (info) *info = out;
    return rc;
}

int nl_stack_frame_location_scale(nl_stack_t *h, int idx, int estimator, int num_samples, const uint32_t *seeds,
                                  int n_seeds, const float *min_max, float *location, float *scale, nl_locscale_t *info)
{
    const char *who = idx < 0 ? "result_location_scale" : "frame_location_scale";
    int rc = locscale_check(who, estimator, num_samples, seeds, n_seeds, location, scale);
    if (rc != NL_OK) return rc;
    float *d;
    if ((rc = resident_entry(h, idx, who, true, &d)) != NL_OK) return rc;
    return locscale_impl(h, d, who, estimator, num_samples, seeds, min_max, location, scale, info);
}

int nl_location_scale(const float *data_host, int width, int height, int estimator, int num_samples,
                      const uint32_t *seeds, int n_seeds, const float *min_max, float *location, float *scale,
                      nl_locscale_t *info, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "location_scale: bad argument");
    int rc = locscale_check("location_scale", estimator, num_samples, seeds, n_seeds, location, scale);
    if (rc != NL_OK) return rc;
    if ((rc = select_device(device)) != NL_OK) return rc;
    return host_frames_run(1, data_host, nullptr, width, height, device, [&](nl_stack_t *h) {
        return locscale_impl(h, h->d_frames, "location_scale", estimator, num_samples, seeds, min_max, location, scale, info);
    });
}

int nl_locscale_seeds(uint64_t key, uint32_t *seeds, int n)
{
    if (n < 0 || (n > 0 && !seeds)) return fail(NL_ERR_INVALID_ARG, "locscale_seeds: %d seeds with no output", n);
    uint64_t x = key;
    for (int i = 0; i < n;) {                                   // splitmix64; the high half, zeros skipped
        uint64_t z = (x += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        if ((uint32_t)(z >> 32) != 0) seeds[i++] = (uint32_t)(z >> 32);
    }
    return NL_OK;
}

int nl_stack_frame_noise(nl_stack_t *h, int idx, float *noise)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    if (idx < 0 || idx >= h->n_frames || !noise)
        return fail(NL_ERR_INVALID_ARG, "frame_noise: bad index %d or null output", idx);
    int rc = need_whole_image(h, "frame_noise", "3x3 stencil");
    if (rc != NL_OK) return rc;
    if (h->width < 3 || h->height < 3) return fail(NL_ERR_INVALID_ARG, "frame_noise: image too small");
    const float *d = h->d_frames + (int64_t)idx * h->fstride;
    NL_HIP(nl::launch_noise(d, h->width, h->height, h->d_stat_partial, kStatBlocks, h->stream));
    double s;
    if ((rc = sum_stat_partials(h, &s)) != NL_OK) return rc;
    // noise.go:53: factor = float32(sqrt(pi/2)) / (6*float32(w-2)*float32(h-2)), fp32
    const float c = (float)sqrt(0.5 * M_PI);
    volatile float den = 6.0f * (float)(h->width - 2);
    den = den * (float)(h->height - 2);
    const float factor = c / den;
    *noise = (float)s * factor;
    return NL_OK;
}

int nl_stack_weights_from_noise(nl_stack_t *h, float *noise_out)
{
    NL_CHECK_HANDLE(h);
    std::vector<float> noise((size_t)h->n_frames), w((size_t)h->n_frames);
    for (int i = 0; i < h->n_frames; i++) {
        int rc = nl_stack_frame_noise(h, i, &noise[(size_t)i]);
        if (rc != NL_OK) return rc;
    }
    if (noise_out) memcpy(noise_out, noise.data(), sizeof(float) * noise.size());
    int rc = nl_weights_from_scalars(NL_WEIGHT_INVERSE_NOISE, noise.data(), h->n_frames, w.data(), nullptr);
    if (rc != NL_OK) return rc;
    return nl_stack_set_weights(h, w.data());
}

int nl_stack_frame_affine(nl_stack_t *h, int idx, float multiplier, float offset)
{
    float *d;
    if (const int rc = resident_entry(h, idx, "frame_affine", false, &d); rc != NL_OK) return rc;
    NL_HIP(nl::launch_affine(d, h->npix, multiplier, offset, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// MedianFilter / GatherAndMedian, ops/pre/badpixels.go:54-77 and internal/median/gather.go:26-38
int nl_median_filter_mask(const float *in_host, float *out_host, int64_t n, const int32_t *mask, int mask_len, int device)
{
    if (!in_host || !out_host || n < 1 || !mask || mask_len < 1 || mask_len > nl::kMedianMaskMax)
        return fail(NL_ERR_INVALID_ARG, "median_filter_mask: bad argument (mask of 1..%d offsets)", nl::kMedianMaskMax);
    return median_filter_run("median_filter_mask", in_host, out_host, n, device, [&](const float *d_in, float *d_out) {
        return nl::launch_median_mask(d_in, d_out, n, mask, mask_len, nullptr);
    });
}

int nl_median_filter_3x3(const float *in_host, float *out_host, int width, int height, int device)
{
    if (!in_host || !out_host || width < 1 || height < 1)
        return fail(NL_ERR_INVALID_ARG, "median_filter_3x3: bad argument");
    return median_filter_run("median_filter_3x3", in_host, out_host, (int64_t)width * height, device,
                             [&](const float *d_in, float *d_out) {
                                 return nl::launch_median3x3(d_in, d_out, width, height, nullptr);
                             });
}

// ---- OpAlign's f.Project from a resident frame (post/postprocess.go:185, fits/project.go:26-76; kernel in project.hip) ----

int nl_stack_frame_project_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float trans[6],
                                float out_of_bounds)
{
    return nl::stack_project_from(dst, dst_idx, src, src_idx, trans, out_of_bounds, "frame_project_from", false);
}

int nl_stack_project_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], int64_t *staged,
                                int64_t *direct)
{
    if (!dst || !src || !trans || !staged || !direct) return fail(NL_ERR_INVALID_ARG, "project_tile_paths: null argument");
    if (src_idx < 0 || src_idx >= src->n_frames)               // (a host query: no device, no stream is touched)
        return fail(NL_ERR_INVALID_ARG, "project_tile_paths: bad index %d", src_idx);
    const float *s = src->d_frames + (int64_t)src_idx * src->fstride;
    float inv[6];
    const int rc = invert_transform(trans, inv);
    if (rc != NL_OK) return rc;
    nl::project_tile_paths(s, src->width, src->height, dst->width, dst->row0, dst->rows, inv, project_switches(dst),
                           staged, direct);
    return NL_OK;
}

// ---- the same projection with a bicubic or Lanczos-3 kernel (include/nlstack_resample.h, an extension; kernels in resample.hip) ----

int nl_resample_lanczos3_table(float *table)
{
    if (!table) return fail(NL_ERR_INVALID_ARG, "resample_lanczos3_table: null table");
    memcpy(table, nl::lanczos3_table_host(), sizeof(float) * NL_RS_PHASES * 6);
    return NL_OK;
}

int nl_stack_frame_resample_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float trans[6],
                                 float out_of_bounds, int kernel, int clamp)
{
    const int rc = nl::resample_args_check("frame_resample_from", kernel, trans);      // in front of any device work
    if (rc != NL_OK) return rc;
    if (!dst || !src) return fail(NL_ERR_INVALID_ARG, "frame_resample_from: null handle");
    return nl::stack_project_from(dst, dst_idx, src, src_idx, trans, out_of_bounds, "frame_resample_from", false, kernel, clamp);
}

int nl_stack_resample_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], int kernel,
                                 int64_t *staged, int64_t *direct)
{
    if (!dst || !src || !trans || !staged || !direct) return fail(NL_ERR_INVALID_ARG, "resample_tile_paths: null argument");
    const int rc = nl::resample_args_check("resample_tile_paths", kernel, trans);
    if (rc != NL_OK) return rc;
    if (kernel == NL_RS_BILINEAR) return nl_stack_project_tile_paths(dst, src, src_idx, trans, staged, direct);
    if (src_idx < 0 || src_idx >= src->n_frames)               // (a host query: no device, no stream is touched)
        return fail(NL_ERR_INVALID_ARG, "resample_tile_paths: bad index %d", src_idx);
    const float *s = src->d_frames + (int64_t)src_idx * src->fstride;
    float inv[6];
    (void)invert_transform(trans, inv);
    nl::resample_tile_paths(s, src->width, src->height, dst->width, dst->row0, dst->rows, inv, kernel + 1,
                            project_switches(dst), staged, direct);
    return NL_OK;
}

}  // extern "C"
