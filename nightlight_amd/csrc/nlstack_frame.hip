// nlstack_frame.hip -- steps on one frame resident in a handle, and their host forms: statistics and noise,
// median filters, OpCalibrate / OpBadPixel, star detection, background extraction, debanding and binning, Gaussian blur
// and unsharp mask, the tone curves and the gray export, the colour steps of the rgb command, the colour-camera front.
// Kernels in frame_stats.hip, preprocess.hip, stars.hip, background.hip, deband.hip, blur.hip, tone.hip, colour.hip and
// bayer.hip.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "bayer.hpp"
#include "preprocess.hpp"
#include "nlstack_internal.hpp"

namespace {

// the per-block {min, sum, max} partials of launch_min_sum_max folded from block 0 on: compared in fp32, summed in
// fp64 in block order (the results are bit-exact against the reference)
struct MinSumMax { float lo; double sum; float hi; };
MinSumMax fold_min_sum_max(const std::vector<double> &part)
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

// ---- what the entry points ask of the handle first (h is checked) ----

// frame idx of the handle; without one nullptr, and "<who>: bad index <idx>" is the thread's error
float *frame_or_fail(nl_stack_t *h, int idx, const char *who)
{
    if (idx < 0 || idx >= h->n_frames) {
        fail(NL_ERR_INVALID_ARG, "%s: bad index %d", who, idx);
        return nullptr;
    }
    return h->d_frames + (int64_t)idx * h->fstride;
}

// a step that looks beyond its own pixel (why) cannot run on a tile of rows
int need_whole_image(const nl_stack_t *h, const char *who, const char *why)
{
    if (h->row0 == 0 && h->rows == h->height) return NL_OK;
    return fail(NL_ERR_INVALID_ARG, "%s needs a whole-image handle (%s)", who, why);
}

// the kernels of these steps index pixels with 32 bits
int need_int32_pixels(int64_t n, const char *who, const char *what = "frame")
{
    if (n < ((int64_t)1 << 31)) return NL_OK;
    return fail(NL_ERR_INVALID_ARG, "%s: %s of 2^31 pixels or more", who, what);
}

}  // namespace

extern "C" {

// ---- per-frame statistics ---------------------------------------------------

// min / mean / max of n values from the {min, sum, max} partials a kernel enqueued on h->stream leaves in
// h->d_stat_partial (launch_min_sum_max, or a tone curve that reduces what it writes) or in d_part; waits for the stream
static int min_mean_max_from_partials(nl_stack_t *h, int64_t n, float *mn, float *mean, float *mx,
                                      const double *d_part = nullptr)
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

static int frame_stats_impl(nl_stack_t *h, const float *d, int64_t n, float *mn, float *mean,
                            float *mx, double *variance)
{
    std::vector<double> part(kStatBlocks);
    float m = 0.0f;
    NL_HIP(nl::launch_min_sum_max(d, n, h->d_stat_partial, kStatBlocks, h->stream));
    const int rc = min_mean_max_from_partials(h, n, mn, &m, mx);
    if (rc != NL_OK) return rc;
    if (mean) *mean = m;
    if (variance) {
        NL_HIP(nl::launch_variance(d, n, m, h->d_stat_partial, kStatBlocks, h->stream));
        NL_HIP(hipMemcpyAsync(part.data(), h->d_stat_partial, sizeof(double) * kStatBlocks,
                              hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
        double s = 0.0;
        for (int b = 0; b < kStatBlocks; b++) s += part[b];
        *variance = s / (double)n;
    }
    return NL_OK;
}

int nl_stack_frame_stats(nl_stack_t *h, int idx, float *mn, float *mean, float *mx,
                         double *variance)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    const float *d = frame_or_fail(h, idx, "frame_stats");
    return d ? frame_stats_impl(h, d, h->npix, mn, mean, mx, variance) : NL_ERR_INVALID_ARG;
}

static int frame_noise_impl(nl_stack_t *h, const float *d, float *noise)
{
    std::vector<double> part(kStatBlocks);
    NL_HIP(nl::launch_noise(d, h->width, h->height, h->d_stat_partial, kStatBlocks, h->stream));
    NL_HIP(hipMemcpyAsync(part.data(), h->d_stat_partial, sizeof(double) * kStatBlocks,
                          hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    double s = 0.0;
    for (int b = 0; b < kStatBlocks; b++) s += part[b];
    // noise.go:53: factor = float32(sqrt(pi/2)) / (6*float32(w-2)*float32(h-2)), fp32
    const float c = (float)sqrt(0.5 * M_PI);
    volatile float den = 6.0f * (float)(h->width - 2);
    den = den * (float)(h->height - 2);
    const float factor = c / den;
    *noise = (float)s * factor;
    return NL_OK;
}

int nl_stack_frame_noise(nl_stack_t *h, int idx, float *noise)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    if (idx < 0 || idx >= h->n_frames || !noise)
        return fail(NL_ERR_INVALID_ARG, "frame_noise: bad index %d or null output", idx);
    const int rc = need_whole_image(h, "frame_noise", "3x3 stencil");
    if (rc != NL_OK) return rc;
    if (h->width < 3 || h->height < 3) return fail(NL_ERR_INVALID_ARG, "frame_noise: image too small");
    return frame_noise_impl(h, h->d_frames + (int64_t)idx * h->fstride, noise);
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
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    float *d = frame_or_fail(h, idx, "frame_affine");
    if (!d) return NL_ERR_INVALID_ARG;
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

// ---- OpCalibrate / OpBadPixel, mono (internal/ops/pre/preprocess.go:68-195; kernels in preprocess.hip) ----------

// OpCalibrate's masters on one device (read-only after nl_calib_create: any number of threads may share one)
struct nl_calib {
    int device = 0;
    int width = 0, height = 0;             // Naxisn of the masters
    float *d_dark = nullptr, *d_flat = nullptr;
    float flat_max = 0.0f;                 // FlatFrame.Stats.Max()
};

// Stats.Max() (stats.go:112-121) of the flat through the min / sum / max reduction of nl_stack_frame_stats
static int flat_max_impl(const float *d_flat, int64_t n, float *out)
{
    double *d_part = nullptr;
    NL_HIP(dev_malloc(&d_part, sizeof(double) * 3 * kStatBlocks));
    std::vector<double> part(3 * kStatBlocks);
    hipError_t e = nl::launch_min_sum_max(d_flat, n, d_part, kStatBlocks, nullptr);
    if (e == hipSuccess) e = hipMemcpy(part.data(), d_part, sizeof(double) * part.size(), hipMemcpyDeviceToHost);
    (void)hipFree(d_part);
    if (e != hipSuccess) return fail(NL_ERR_HIP, "calib_create: flat maximum: %s", hipGetErrorString(e));
    *out = fold_min_sum_max(part).hi;
    return NL_OK;
}

static int calib_create_impl(nl_calib *c, const float *dark_host, const float *flat_host)
{
    int rc = select_device(c->device);
    if (rc != NL_OK) return rc;
    const int64_t n = (int64_t)c->width * c->height;
    const size_t bytes = (size_t)n * sizeof(float);
    if (dark_host) {
        NL_HIP(dev_malloc(&c->d_dark, bytes));
        NL_HIP(hipMemcpy(c->d_dark, dark_host, bytes, hipMemcpyHostToDevice));
    }
    if (flat_host) {
        NL_HIP(dev_malloc(&c->d_flat, bytes));
        NL_HIP(hipMemcpy(c->d_flat, flat_host, bytes, hipMemcpyHostToDevice));
        return flat_max_impl(c->d_flat, n, &c->flat_max);
    }
    return NL_OK;
}

nl_calib_t *nl_calib_create(int device, const float *dark_host, int dark_width, int dark_height,
                            const float *flat_host, int flat_width, int flat_height)
{
    if (!dark_host && !flat_host) { fail(NL_ERR_INVALID_ARG, "calib_create: neither a dark nor a flat"); return nullptr; }
    if ((dark_host && (dark_width < 1 || dark_height < 1)) || (flat_host && (flat_width < 1 || flat_height < 1))) {
        fail(NL_ERR_INVALID_ARG, "calib_create: bad master dimensions");
        return nullptr;
    }
    if (dark_host && flat_host && (dark_width != flat_width || dark_height != flat_height)) {      // preprocess.go:144-147
        fail(NL_ERR_INVALID_ARG, "dark dimensions [%d %d] differ from flat dimensions [%d %d]", dark_width, dark_height,
             flat_width, flat_height);
        return nullptr;
    }
    nl_calib *c = new nl_calib();
    c->device = device;
    c->width = dark_host ? dark_width : flat_width;
    c->height = dark_host ? dark_height : flat_height;
    if (calib_create_impl(c, dark_host, flat_host) != NL_OK) {
        std::string keep = g_err;
        nl_calib_destroy(c);
        g_err = keep;
        return nullptr;
    }
    return c;
}

void nl_calib_destroy(nl_calib_t *c)
{
    if (!c) return;
    if (c->d_dark || c->d_flat) {
        (void)hipSetDevice(c->device);
        if (c->d_dark) (void)hipFree(c->d_dark);
        if (c->d_flat) (void)hipFree(c->d_flat);
    }
    delete c;
}

int nl_calib_flat_max(const nl_calib_t *c, float *out)
{
    if (!c || !out) return fail(NL_ERR_INVALID_ARG, "calib_flat_max: null argument");
    if (!c->d_flat) return fail(NL_ERR_INVALID_ARG, "calib_flat_max: the calibration has no flat");
    *out = c->flat_max;
    return NL_OK;
}

// preprocess.go:73-93: the masters' shape, or another one with the same pixel count (the Seestar case: the data is
// taken as 1-D, the reference prints a warning), else the reference's error (the dark is checked first)
static int calib_check_light(const nl_calib *c, int frame_id, int width, int height)
{
    if ((width == c->width && height == c->height) || (int64_t)width * height == (int64_t)c->width * c->height)
        return NL_OK;
    return fail(NL_ERR_INVALID_ARG, "%d: Light dimensions [%d %d] differ from %s dimensions [%d %d]", frame_id, width,
                height, c->d_dark ? "dark" : "flat", c->width, c->height);
}

int nl_stack_frame_calibrate(nl_stack_t *h, int idx, const nl_calib_t *c)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    if (idx < 0 || idx >= h->n_frames || !c)
        return fail(NL_ERR_INVALID_ARG, "frame_calibrate: bad index %d or null calibration", idx);
    if (c->device != h->device)
        return fail(NL_ERR_INVALID_ARG, "frame_calibrate: calibration on device %d, handle on device %d", c->device,
                    h->device);
    int rc = calib_check_light(c, idx, h->width, h->height);
    if (rc != NL_OK) return rc;
    const int64_t off = (int64_t)h->row0 * h->width;          // the tile's 1-D range of the masters
    float *d = h->d_frames + (int64_t)idx * h->fstride;
    NL_HIP(nl::launch_calibrate(d, d, h->npix, c->d_dark ? c->d_dark + off : nullptr,
                                c->d_flat ? c->d_flat + off : nullptr, c->flat_max, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl_stack_frame_badpixel(nl_stack_t *h, int idx, float sigma_low, float sigma_high, int64_t *removed_out,
                            float *diff_stats_out)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    float *d = frame_or_fail(h, idx, "frame_badpixel");
    if (!d) return NL_ERR_INVALID_ARG;
    if (sigma_low == 0.0f || sigma_high == 0.0f) {         // preprocess.go:181-183: nothing to do
        if (removed_out) *removed_out = 0;
        if (diff_stats_out) diff_stats_out[0] = diff_stats_out[1] = NAN;
        return NL_OK;
    }
    if (sigma_low < 0.0f || sigma_high < 0.0f)             // (the reference would flag the border: not supported)
        return fail(NL_ERR_INVALID_ARG, "frame_badpixel: negative sigma (low %g, high %g)", sigma_low, sigma_high);
    int rc = need_whole_image(h, "frame_badpixel", "3x3 stencil, whole-frame std");
    if (rc == NL_OK) rc = need_int32_pixels(h->npix, "frame_badpixel");
    if (rc != NL_OK) return rc;
    const int blocks = nl::bp_blocks(h->npix);
    nl_stack::FrameScratch &fs = h->frame_scratch;
    NL_HIP(fs.bp_diff.reserve(sizeof(float) * (size_t)h->npix, h->device));
    NL_HIP(fs.bp_seg.reserve(sizeof(unsigned) * (size_t)blocks * nl::kBpChunk, h->device));
    NL_HIP(fs.bp_list.reserve(sizeof(unsigned) * (size_t)h->npix, h->device));
    NL_HIP(fs.bp_small.reserve(sizeof(nl::BpParams) + 3 * sizeof(unsigned) * (size_t)blocks, h->stream));
    nl::BpScratch s;
    s.diff = static_cast<float *>(fs.bp_diff.ptr);
    s.seg = static_cast<unsigned *>(fs.bp_seg.ptr);
    s.list = static_cast<unsigned *>(fs.bp_list.ptr);
    s.params = static_cast<nl::BpParams *>(fs.bp_small.ptr);
    s.count = reinterpret_cast<unsigned *>(s.params + 1);
    s.offset = s.count + blocks;
    s.removed = s.offset + blocks;
    s.partial = h->d_stat_partial;
    s.stat_blocks = kStatBlocks;
    NL_HIP(nl::launch_badpixel(d, h->width, h->height, sigma_low, sigma_high, s, h->stream));
    nl::BpParams p;
    NL_HIP(hipMemcpyAsync(&p, s.params, sizeof p, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    if (removed_out) *removed_out = (int64_t)p.removed;
    if (diff_stats_out) { diff_stats_out[0] = p.mean; diff_stats_out[1] = p.std; }
    return NL_OK;
}

// what both preprocess host forms check first: the arguments, the device, the calibration's device and shape
static int preprocess_check(const char *who, const nl_calib *c, int frame_id, const float *in_host, const float *out_host,
                            int width, int height, int device)
{
    if (!in_host || !out_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "%s: bad argument", who);
    const int rc = select_device(device);
    if (rc != NL_OK) return rc;
    if (c && c->device != device)
        return fail(NL_ERR_INVALID_ARG, "%s: calibration on device %d, frame on device %d", who, c->device, device);
    return c ? calib_check_light(c, frame_id, width, height) : NL_OK;
}

int nl_preprocess_frame(const nl_calib_t *c, int frame_id, const float *in_host, float *out_host, int width, int height,
                        float sigma_low, float sigma_high, int64_t *removed_out, float *diff_stats_out, int device)
{
    const int rc = preprocess_check("preprocess_frame", c, frame_id, in_host, out_host, width, height, device);
    if (rc != NL_OK) return rc;
    return with_scratch_handle(width, height, device, [&](nl_stack_t *h) {
        int r = nl_stack_upload_tile(h, 0, in_host);
        if (r == NL_OK && c) r = nl_stack_frame_calibrate(h, 0, c);
        if (r == NL_OK) r = nl_stack_frame_badpixel(h, 0, sigma_low, sigma_high, removed_out, diff_stats_out);
        return r == NL_OK ? nl_stack_download_tile(h, 0, out_host) : r;
    });
}

// ---- OpStarDetect: star.FindStars (internal/star/findstars.go:59-103; kernels and host steps in stars.hip) ---------

static int find_stars_impl(nl_stack_t *h, const float *d_data, const char *who, float location, float scale,
                           float star_sig, float bp_sigma, float star_in_out, int radius, float diff_std,
                           nl_star_t *stars_out, int capacity, int *n_stars, float *sum_of_shifts, float *avg_hfr)
{
    if (radius < 0 || radius > 1024)      // (deviation 2; radius 0 finds no star)
        return fail(NL_ERR_INVALID_ARG, "%s: radius %d not in [0, 1024]", who, radius);
    if (capacity < 0 || (capacity > 0 && !stars_out))
        return fail(NL_ERR_INVALID_ARG, "%s: capacity %d with %s output", who, capacity, stars_out ? "an" : "no");
    int pre = need_whole_image(h, who, "FindStars indexes the data 1-D");
    if (pre == NL_OK) pre = need_int32_pixels(h->npix, who);
    if (pre != NL_OK) return pre;
    if (!h->d_stat_partial) NL_HIP(dev_malloc(&h->d_stat_partial, sizeof(double) * 3 * kStatBlocks));
    const nl::StarParams p{location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std};
    std::vector<nl_star_t> stars;
    float sum = 0.0f, avg = 0.0f;
    std::string msg;
    const int rc = nl::find_stars_run(d_data, h->width, h->height, p, h->frame_scratch.star_work, h->d_stat_partial, kStatBlocks,
                                      h->stream, stars, &sum, &avg, &msg);
    if (rc != NL_OK) return fail(rc, "%s: %s", who, msg.c_str());
    const size_t k = std::min(stars.size(), (size_t)capacity);
    if (k) memcpy(stars_out, stars.data(), k * sizeof(nl_star_t));
    if (n_stars) *n_stars = (int)stars.size();
    if (sum_of_shifts) *sum_of_shifts = sum;
    if (avg_hfr) *avg_hfr = avg;
    return NL_OK;
}

int nl_stack_frame_find_stars(nl_stack_t *h, int idx, float location, float scale, float star_sig, float bp_sigma,
                              float star_in_out, int radius, float diff_std, nl_star_t *stars_out, int capacity,
                              int *n_stars, float *sum_of_shifts, float *avg_hfr)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    const float *d = frame_or_fail(h, idx, "frame_find_stars");
    if (!d) return NL_ERR_INVALID_ARG;
    return find_stars_impl(h, d, "frame_find_stars", location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std,
                           stars_out, capacity, n_stars, sum_of_shifts, avg_hfr);
}

int nl_stack_result_find_stars(nl_stack_t *h, float location, float scale, float star_sig, float bp_sigma,
                               float star_in_out, int radius, float diff_std, nl_star_t *stars_out, int capacity,
                               int *n_stars, float *sum_of_shifts, float *avg_hfr)
{
    NL_CHECK_HANDLE(h);
    if (h->last_mode < 0) return fail(NL_ERR_INVALID_ARG, "result_find_stars: the handle has not run a pass");
    return find_stars_impl(h, h->d_out, "result_find_stars", location, scale, star_sig, bp_sigma, star_in_out, radius,
                           diff_std, stars_out, capacity, n_stars, sum_of_shifts, avg_hfr);
}

int nl_find_stars(const float *data_host, int width, int height, float location, float scale, float star_sig,
                  float bp_sigma, float star_in_out, int radius, float diff_std, nl_star_t *stars_out, int capacity,
                  int *n_stars, float *sum_of_shifts, float *avg_hfr, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "find_stars: bad argument");
    const int rc = select_device(device);
    if (rc != NL_OK) return rc;
    return with_scratch_handle(width, height, device, [&](nl_stack_t *h) {
        const int r = nl_stack_upload_tile(h, 0, data_host);
        if (r != NL_OK) return r;
        return find_stars_impl(h, h->d_frames, "find_stars", location, scale, star_sig, bp_sigma, star_in_out, radius,
                               diff_std, stars_out, capacity, n_stars, sum_of_shifts, avg_hfr);
    });
}

// ---- OpBackExtract: pre.NewBackground + Subtract / Render (internal/ops/pre/background.go:68-462; background.hip) --

static int back_extract_impl(nl_stack_t *h, float *d_data, const char *who, int grid_size, float hfr_factor,
                             float sigma, int clip, const nl_star_t *stars, int n_stars, float *background_out,
                             float *cells_out, int cells_capacity, nl_background_t *info)
{
    if (n_stars < 0 || (n_stars > 0 && !stars)) return fail(NL_ERR_INVALID_ARG, "%s: %d stars", who, n_stars);
    if (cells_capacity < 0 || (cells_capacity > 0 && !cells_out))
        return fail(NL_ERR_INVALID_ARG, "%s: capacity %d with %s output", who, cells_capacity, cells_out ? "an" : "no");
    int pre = need_whole_image(h, who, "the grid spans the whole frame");
    if (pre == NL_OK) pre = need_int32_pixels(h->npix, who);
    if (pre != NL_OK) return pre;
    if (grid_size <= 0) {                  // OpBackExtract.Apply is a no-op (preprocess.go:373-375)
        if (info) memset(info, 0, sizeof *info);
        return NL_OK;
    }
    const nl::BackParams p{grid_size, hfr_factor, sigma, clip};
    std::string msg;
    const int rc = nl::back_extract_run(d_data, h->width, h->height, p, stars, n_stars, h->frame_scratch.back_work,
                                        h->stream, background_out, cells_out, cells_capacity, info, &msg);
    return rc == NL_OK ? NL_OK : fail(rc, "%s: %s", who, msg.c_str());
}

int nl_stack_frame_back_extract(nl_stack_t *h, int idx, int grid_size, float hfr_factor, float sigma, int clip,
                                const nl_star_t *stars, int n_stars, float *background_out, float *cells_out,
                                int cells_capacity, nl_background_t *info)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    float *d = frame_or_fail(h, idx, "frame_back_extract");
    if (!d) return NL_ERR_INVALID_ARG;
    return back_extract_impl(h, d, "frame_back_extract", grid_size, hfr_factor, sigma, clip, stars, n_stars,
                             background_out, cells_out, cells_capacity, info);
}

int nl_back_extract(float *data_host, int width, int height, int grid_size, float hfr_factor, float sigma, int clip,
                    const nl_star_t *stars, int n_stars, float *background_out, float *cells_out, int cells_capacity,
                    nl_background_t *info, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "back_extract: bad argument");
    const int rc = select_device(device);
    if (rc != NL_OK) return rc;
    if (grid_size <= 0)                    // no-op: the frame is not even uploaded
        return with_scratch_handle(1, 1, device, [&](nl_stack_t *h) {
            return back_extract_impl(h, h->d_frames, "back_extract", grid_size, hfr_factor, sigma, clip, stars,
                                     n_stars, background_out, cells_out, cells_capacity, info);
        });
    return with_scratch_handle(width, height, device, [&](nl_stack_t *h) {
        int r = nl_stack_upload_tile(h, 0, data_host);
        if (r == NL_OK)
            r = back_extract_impl(h, h->d_frames, "back_extract", grid_size, hfr_factor, sigma, clip, stars, n_stars,
                                  background_out, cells_out, cells_capacity, info);
        return r == NL_OK ? nl_stack_download_tile(h, 0, data_host) : r;
    });
}

// ---- OpDebandHoriz / OpDebandVert (internal/ops/pre/banding.go:61-270; kernels and host steps in deband.hip) -------

// the operators' own guards (:62, :198)
static bool deband_is_noop(bool cols, float percentile, int window)
{
    return percentile <= 0.0f || percentile >= 100.0f || (!cols && window <= 0);
}

static int deband_impl(nl_stack_t *h, float *d_data, const char *who, bool cols, float percentile, int window,
                       float sigma, float location, float scale, nl_deband_t *info)
{
    int pre = need_whole_image(h, who, "the window needs every row's percentile");
    if (pre == NL_OK) pre = need_int32_pixels(h->npix, who);
    if (pre != NL_OK) return pre;
    float threshold = FLT_MAX;                 // :75-79, :211-215
    if (sigma != 0.0f) threshold = location + sigma * scale;
    nl_deband_t out{threshold, 1.0f, 0.0f};
    if (!deband_is_noop(cols, percentile, window)) {
        const nl::DebandParams p{percentile, window, threshold};
        std::string msg;
        const int rc = nl::deband_run(d_data, h->width, h->height, cols, p, h->frame_scratch.deband_work, h->stream,
                                      &out.lowest, &out.highest, &msg);
        if (rc != NL_OK) return fail(rc, "%s: %s", who, msg.c_str());
    }
    if (info) *info = out;
    return NL_OK;
}

static int frame_deband(nl_stack_t *h, int idx, const char *who, bool cols, float percentile, int window, float sigma,
                        float location, float scale, nl_deband_t *info)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    float *d = frame_or_fail(h, idx, who);
    if (!d) return NL_ERR_INVALID_ARG;
    return deband_impl(h, d, who, cols, percentile, window, sigma, location, scale, info);
}

int nl_stack_frame_deband_horiz(nl_stack_t *h, int idx, float percentile, int window, float sigma, float location,
                                float scale, nl_deband_t *info)
{
    return frame_deband(h, idx, "frame_deband_horiz", false, percentile, window, sigma, location, scale, info);
}

int nl_stack_frame_deband_vert(nl_stack_t *h, int idx, float percentile, int window, float sigma, float location,
                               float scale, nl_deband_t *info)
{
    return frame_deband(h, idx, "frame_deband_vert", true, percentile, window, sigma, location, scale, info);
}

static int host_deband(float *data_host, int width, int height, const char *who, bool cols, float percentile,
                       int window, float sigma, float location, float scale, nl_deband_t *info, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "%s: bad argument", who);
    const int rc = select_device(device);
    if (rc != NL_OK) return rc;
    if (deband_is_noop(cols, percentile, window))      // no-op: the frame is not even uploaded
        return with_scratch_handle(1, 1, device, [&](nl_stack_t *h) {
            return deband_impl(h, h->d_frames, who, cols, percentile, window, sigma, location, scale, info);
        });
    return with_scratch_handle(width, height, device, [&](nl_stack_t *h) {
        int r = nl_stack_upload_tile(h, 0, data_host);
        if (r == NL_OK) r = deband_impl(h, h->d_frames, who, cols, percentile, window, sigma, location, scale, info);
        return r == NL_OK ? nl_stack_download_tile(h, 0, data_host) : r;
    });
}

int nl_deband_horiz(float *data_host, int width, int height, float percentile, int window, float sigma,
                    float location, float scale, nl_deband_t *info, int device)
{
    return host_deband(data_host, width, height, "deband_horiz", false, percentile, window, sigma, location, scale,
                       info, device);
}

int nl_deband_vert(float *data_host, int width, int height, float percentile, int window, float sigma, float location,
                   float scale, nl_deband_t *info, int device)
{
    return host_deband(data_host, width, height, "deband_vert", true, percentile, window, sigma, location, scale,
                       info, device);
}

// ---- OpBin: fits.NewImageBinNxN (internal/ops/pre/preprocess.go:324-331, internal/fits/fits.go:163-195; deband.hip) -

int nl_bin_shape(int width, int height, int n, int *out_width, int *out_height)
{
    if (width < 1 || height < 1 || !out_width || !out_height) return fail(NL_ERR_INVALID_ARG, "bin_shape: bad argument");
    if (n <= 1) {                              // OpBin.Apply is a no-op (preprocess.go:325-327)
        *out_width = width;
        *out_height = height;
        return NL_OK;
    }
    *out_width = width / n;                    // fits.go:167-171
    *out_height = height / n;
    if (*out_width == 0 || *out_height == 0)   // (deviation)
        return fail(NL_ERR_INVALID_ARG, "NewImageBinNxN (fits.go:163-195): %dx%d binned by %d gives an empty %dx%d image",
                    width, height, n, *out_width, *out_height);
    return NL_OK;
}

int nl_stack_frame_bin_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, int n)
{
    NL_CHECK_HANDLE(src);
    NL_CHECK_HANDLE(dst);
    if (src->device != dst->device)
        return fail(NL_ERR_INVALID_ARG, "frame_bin_from: source on device %d, destination on device %d", src->device,
                    dst->device);
    NL_SETTLE_UPLOADS(src);
    NL_SETTLE_UPLOADS(dst);
    const float *s = frame_or_fail(src, src_idx, "frame_bin_from (source)");
    float *d = s ? frame_or_fail(dst, dst_idx, "frame_bin_from (destination)") : nullptr;
    if (!d) return NL_ERR_INVALID_ARG;
    int rc = need_whole_image(src, "frame_bin_from (source)", "a bin spans rows");
    if (rc == NL_OK) rc = need_whole_image(dst, "frame_bin_from (destination)", "a bin spans rows");
    if (rc == NL_OK) rc = need_int32_pixels(src->npix, "frame_bin_from");
    if (rc != NL_OK) return rc;
    if (dst->d_frames != dst->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "frame_bin_from: the destination's frames are attached, not owned");
    int ow, oh;
    if ((rc = nl_bin_shape(src->width, src->height, n, &ow, &oh)) != NL_OK) return rc;
    if (dst->width != ow || dst->height != oh)
        return fail(NL_ERR_INVALID_ARG, "frame_bin_from: %dx%d binned by %d is %dx%d, the destination is %dx%d",
                    src->width, src->height, n, ow, oh, dst->width, dst->height);
    if (src != dst && (rc = nl_stack_order_stream_after(src, dst->stream)) != NL_OK) return rc;
    if (n > 1)
        NL_HIP(nl::launch_bin(s, src->width, src->height, n, d, dst->stream));
    else if (s != d)
        NL_HIP(hipMemcpyAsync(d, s, sizeof(float) * (size_t)src->npix, hipMemcpyDeviceToDevice, dst->stream));
    NL_HIP(hipStreamSynchronize(dst->stream));
    return NL_OK;
}

// ---- OpGaussianBlur / OpUnsharpMask (internal/ops/stretch/stretch.go:339-424, usm.go; kernels in blur.hip) ---------

int nl_gaussian_kernel_1d(float sigma, float *taps_out, int capacity, int *n_taps_out)
{
    if (capacity < 0 || (capacity > 0 && !taps_out))
        return fail(NL_ERR_INVALID_ARG, "gaussian_kernel_1d: capacity %d with %s output", capacity, taps_out ? "an" : "no");
    std::vector<float> taps;
    std::string msg;
    const int rc = nl::gaussian_kernel_1d(sigma, taps, &msg);
    if (rc != NL_OK) return fail(rc, "gaussian_kernel_1d: %s", msg.c_str());
    if (n_taps_out) *n_taps_out = (int)taps.size();
    if ((size_t)capacity < taps.size())
        return fail(NL_ERR_INVALID_ARG, "gaussian_kernel_1d: sigma %g gives %zu taps, capacity %d", sigma, taps.size(), capacity);
    memcpy(taps_out, taps.data(), sizeof(float) * taps.size());
    return NL_OK;
}

int nl_blur_tap_paths(int n_taps, int *row_staged, int *col_staged)
{
    if (n_taps < 1 || n_taps % 2 == 0 || !row_staged || !col_staged)
        return fail(NL_ERR_INVALID_ARG, "blur_tap_paths: bad argument");
    *row_staged = n_taps / 2 <= nl::kBlurRowStagedRadius;
    *col_staged = n_taps / 2 <= nl::kBlurColStagedRadius;
    return NL_OK;
}

// what every sigma form decides before it touches a device: the operator's own guard (*noop), else the taps of sigma
static int blur_taps(const char *who, float sigma, const nl::UsmParams *usm, std::vector<float> &taps, bool *noop)
{
    *noop = sigma == 0.0f || (usm && usm->gain == 0.0f);      // stretch.go:369, :414
    if (*noop) return NL_OK;
    std::string msg;
    const int rc = nl::gaussian_kernel_1d(sigma, taps, &msg);
    if (rc != NL_OK) return fail(rc, "%s: %s", who, msg.c_str());
    return NL_OK;
}

// deviations 2 and 3, before any device work
static int blur_check_taps(const char *who, const float *taps, int n_taps, int width, int height)
{
    if (!taps || n_taps < 1 || n_taps % 2 == 0)
        return fail(NL_ERR_INVALID_ARG, "%s: %d taps: Convolve1DX / Convolve1DY (usm.go:85-114) index kernel[i + k] for "
                    "i = -k .. k, an odd positive count", who, n_taps);
    if (n_taps / 2 > width || n_taps / 2 > height)
        return fail(NL_ERR_INVALID_ARG, "%s: a radius of %d on a %dx%d frame: one reflect (usm.go:25-33) leaves the range",
                    who, n_taps / 2, width, height);
    return NL_OK;
}

// the two passes on a frame or result resident in h, in place
static int blur_impl(nl_stack_t *h, float *d_data, const char *who, const float *taps, int n_taps,
                     const nl::UsmParams *usm)
{
    int pre = need_whole_image(h, who, "the column pass needs every row");
    if (pre == NL_OK) pre = need_int32_pixels(h->npix, who);
    if (pre == NL_OK) pre = blur_check_taps(who, taps, n_taps, h->width, h->height);
    if (pre != NL_OK) return pre;
    std::string msg;
    const int rc = nl::blur_run(d_data, h->width, h->height, taps, n_taps, usm, h->frame_scratch.blur_work, h->stream, &msg);
    return rc == NL_OK ? NL_OK : fail(rc, "%s: %s", who, msg.c_str());
}

// the resident sigma forms: idx >= 0 a frame slot, idx < 0 the last pass's result
static int resident_blur(nl_stack_t *h, int idx, const char *who, float sigma, const nl::UsmParams *usm)
{
    NL_CHECK_HANDLE(h);
    float *d = h->d_out;
    if (idx >= 0) {
        NL_SETTLE_UPLOADS(h);
        if (!(d = frame_or_fail(h, idx, who))) return NL_ERR_INVALID_ARG;
    } else if (h->last_mode < 0) {
        return fail(NL_ERR_INVALID_ARG, "%s: the handle has not run a pass", who);
    }
    std::vector<float> taps;
    bool noop;
    const int rc = blur_taps(who, sigma, usm, taps, &noop);
    if (rc != NL_OK || noop) return rc;
    return blur_impl(h, d, who, taps.data(), (int)taps.size(), usm);
}

int nl_stack_frame_gaussian_blur(nl_stack_t *h, int idx, float sigma)
{
    if (h && idx < 0) return fail(NL_ERR_INVALID_ARG, "frame_gaussian_blur: bad index %d", idx);
    return resident_blur(h, idx, "frame_gaussian_blur", sigma, nullptr);
}

int nl_stack_frame_unsharp_mask(nl_stack_t *h, int idx, float sigma, float gain, float min, float max,
                                float abs_threshold)
{
    if (h && idx < 0) return fail(NL_ERR_INVALID_ARG, "frame_unsharp_mask: bad index %d", idx);
    const nl::UsmParams p{gain, min, max, abs_threshold};
    return resident_blur(h, idx, "frame_unsharp_mask", sigma, &p);
}

int nl_stack_result_gaussian_blur(nl_stack_t *h, float sigma)
{
    return resident_blur(h, -1, "result_gaussian_blur", sigma, nullptr);
}

int nl_stack_result_unsharp_mask(nl_stack_t *h, float sigma, float gain, float min, float max, float abs_threshold)
{
    const nl::UsmParams p{gain, min, max, abs_threshold};
    return resident_blur(h, -1, "result_unsharp_mask", sigma, &p);
}

// the host forms: the frame up, the two passes on a handle of the call's own, the frame down into out_host
static int host_blur(const char *who, const float *in_host, float *out_host, int width, int height, const float *taps,
                     int n_taps, const nl::UsmParams *usm, int device)
{
    int rc = blur_check_taps(who, taps, n_taps, width, height);
    if (rc == NL_OK) rc = select_device(device);
    if (rc != NL_OK) return rc;
    return with_scratch_handle(width, height, device, [&](nl_stack_t *h) {
        int r = nl_stack_upload_tile(h, 0, in_host);
        if (r == NL_OK) r = blur_impl(h, h->d_frames, who, taps, n_taps, usm);
        return r == NL_OK ? nl_stack_download_tile(h, 0, out_host) : r;
    });
}

int nl_convolve_separable(float *data_host, int width, int height, const float *taps, int n_taps, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "convolve_separable: bad argument");
    return host_blur("convolve_separable", data_host, data_host, width, height, taps, n_taps, nullptr, device);
}

int nl_gaussian_blur(float *data_host, int width, int height, float sigma, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "gaussian_blur: bad argument");
    std::vector<float> taps;
    bool noop;
    const int rc = blur_taps("gaussian_blur", sigma, nullptr, taps, &noop);
    if (rc != NL_OK || noop) return rc;
    return host_blur("gaussian_blur", data_host, data_host, width, height, taps.data(), (int)taps.size(), nullptr, device);
}

int nl_unsharp_mask(const float *in_host, float *out_host, int width, int height, float sigma, float gain, float min,
                    float max, float abs_threshold, int device)
{
    if (!in_host || !out_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "unsharp_mask: bad argument");
    const nl::UsmParams p{gain, min, max, abs_threshold};
    std::vector<float> taps;
    bool noop;
    const int rc = blur_taps("unsharp_mask", sigma, &p, taps, &noop);
    if (rc != NL_OK) return rc;
    if (noop) {
        if (out_host != in_host) memmove(out_host, in_host, sizeof(float) * (size_t)width * height);
        return NL_OK;
    }
    return host_blur("unsharp_mask", in_host, out_host, width, height, taps.data(), (int)taps.size(), &p, device);
}

// ---- the tone curves of the stretch command and OpSave's quantisation (stretch.go:40-335, pixelops.go, tiff16.go,
// writejpg.go; kernels in tone.hip).  Per-pixel steps: a row-tile handle is served, its tile only. ------------------

// the curve over the npix floats at d (a slot or the result of h), in place
static int tone_impl(nl_stack_t *h, float *d, const char *who, const nl_tone_t *tone, float *mn, float *mean, float *mx)
{
    nl::ToneArgs args;
    bool noop;
    std::string msg;
    const int rc = nl::tone_args(*tone, &args, &noop, &msg);
    if (rc != NL_OK) return fail(rc, "%s: %s", who, msg.c_str());
    const bool stats = mn || mean || mx;
    if (noop) return stats ? frame_stats_impl(h, d, h->npix, mn, mean, mx, nullptr) : NL_OK;
    if (!stats) {
        NL_HIP(nl::launch_tone(d, h->npix, args, nullptr, nullptr, 0, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
        return NL_OK;
    }
    nl::DevBuffer &seed = h->frame_scratch.tone_seed;
    NL_HIP(seed.reserve(sizeof(float), h->stream));
    NL_HIP(nl::launch_tone(d, h->npix, args, static_cast<float *>(seed.ptr), h->d_stat_partial, kStatBlocks, h->stream));
    return min_mean_max_from_partials(h, h->npix, mn, mean, mx);
}

// the counts of the npix floats at d into out_host, through the handle's ingest buffer like nl_stack_download_result_fits
static int export_gray_impl(nl_stack_t *h, const float *d, float min, float max, float gamma, int bits, void *out_host)
{
    const float scale = 1.0f / (max - min);                    // tiff16.go:112-113
    const double gamma_inv = (double)(1.0f / gamma);
    const size_t bytes = (size_t)h->npix * (size_t)(bits / 8);
    NL_HIP(h->ingest.reserve(bytes, h->stream));
    NL_HIP(nl::launch_export_gray(d, h->npix, min, scale, gamma_inv != 1.0, gamma_inv, bits, h->ingest.ptr, h->stream));
    NL_HIP(hipMemcpyAsync(out_host, h->ingest.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// what needs no device: the curve's kind (and *noop: the operator's own guard holds)
static int tone_check(const char *who, const nl_tone_t *tone, bool *noop)
{
    if (!tone) return fail(NL_ERR_INVALID_ARG, "%s: null curve", who);
    nl::ToneArgs args;
    std::string msg;
    const int rc = nl::tone_args(*tone, &args, noop, &msg);
    return rc == NL_OK ? NL_OK : fail(rc, "%s: %s", who, msg.c_str());
}

static int export_gray_check(const char *who, float gamma, int bits, const void *out_host)
{
    if (!out_host) return fail(NL_ERR_INVALID_ARG, "%s: null output", who);
    if (bits != 8 && bits != 16) return fail(NL_ERR_INVALID_ARG, "%s: %d bits (8: image.Gray, 16: image.Gray16)", who, bits);
    if (!(gamma > 0.0f))                       // (deviation: gray becomes infinite or NaN in front of the conversion)
        return fail(NL_ERR_INVALID_ARG, "%s: gamma %g (tiff16.go:113, writejpg.go:111: a positive number)", who, gamma);
    return NL_OK;
}

// idx >= 0 a frame slot, idx < 0 the last pass's result (as resident_blur); nullptr with the thread's error set
static float *resident_pixels(nl_stack_t *h, int idx, const char *who, int *rc)
{
    *rc = NL_ERR_INVALID_ARG;
    if (idx >= 0) return frame_or_fail(h, idx, who);
    if (h->last_mode < 0) {
        fail(NL_ERR_INVALID_ARG, "%s: the handle has not run a pass", who);
        return nullptr;
    }
    return h->d_out;
}

static int resident_tone(nl_stack_t *h, int idx, const char *who, const nl_tone_t *tone, float *mn, float *mean, float *mx)
{
    NL_CHECK_HANDLE(h);
    bool noop;
    int rc = tone_check(who, tone, &noop);
    if (rc != NL_OK) return rc;
    if (idx >= 0) NL_SETTLE_UPLOADS(h);
    float *d = resident_pixels(h, idx, who, &rc);
    return d ? tone_impl(h, d, who, tone, mn, mean, mx) : rc;
}

static int resident_export_gray(nl_stack_t *h, int idx, const char *who, float min, float max, float gamma, int bits,
                                void *out_host)
{
    NL_CHECK_HANDLE(h);
    int rc = export_gray_check(who, gamma, bits, out_host);
    if (rc != NL_OK) return rc;
    if (idx >= 0) NL_SETTLE_UPLOADS(h);
    const float *d = resident_pixels(h, idx, who, &rc);
    return d ? export_gray_impl(h, d, min, max, gamma, bits, out_host) : rc;
}

int nl_stack_frame_tone(nl_stack_t *h, int idx, const nl_tone_t *tone, float *mn, float *mean, float *mx)
{
    if (h && idx < 0) return fail(NL_ERR_INVALID_ARG, "frame_tone: bad index %d", idx);
    return resident_tone(h, idx, "frame_tone", tone, mn, mean, mx);
}

int nl_stack_result_tone(nl_stack_t *h, const nl_tone_t *tone, float *mn, float *mean, float *mx)
{
    return resident_tone(h, -1, "result_tone", tone, mn, mean, mx);
}

int nl_stack_frame_export_gray(nl_stack_t *h, int idx, float min, float max, float gamma, int bits, void *out_host)
{
    if (h && idx < 0) return fail(NL_ERR_INVALID_ARG, "frame_export_gray: bad index %d", idx);
    return resident_export_gray(h, idx, "frame_export_gray", min, max, gamma, bits, out_host);
}

int nl_stack_result_export_gray(nl_stack_t *h, float min, float max, float gamma, int bits, void *out_host)
{
    return resident_export_gray(h, -1, "result_export_gray", min, max, gamma, bits, out_host);
}

// the host forms: n floats as an n x 1 frame of a handle of the call's own (like nl_fits_decode)
int nl_tone(float *data_host, int64_t n, const nl_tone_t *tone, float *mn, float *mean, float *mx, int device)
{
    if (!data_host || n < 1 || n > 0x7fffffff) return fail(NL_ERR_INVALID_ARG, "tone: bad argument");
    bool noop;
    int rc = tone_check("tone", tone, &noop);
    if (rc != NL_OK) return rc;
    if (noop && !mn && !mean && !mx) return NL_OK;             // nothing to compute: the frame is not even uploaded
    if ((rc = select_device(device)) != NL_OK) return rc;
    return with_scratch_handle((int)n, 1, device, [&](nl_stack_t *h) {
        int r = nl_stack_upload_tile(h, 0, data_host);
        if (r == NL_OK) r = tone_impl(h, h->d_frames, "tone", tone, mn, mean, mx);
        return r == NL_OK ? nl_stack_download_tile(h, 0, data_host) : r;
    });
}

int nl_export_gray(const float *data_host, int64_t n, float min, float max, float gamma, int bits, void *out_host,
                   int device)
{
    if (!data_host || n < 1 || n > 0x7fffffff) return fail(NL_ERR_INVALID_ARG, "export_gray: bad argument");
    int rc = export_gray_check("export_gray", gamma, bits, out_host);
    if (rc == NL_OK) rc = select_device(device);
    if (rc != NL_OK) return rc;
    return with_scratch_handle((int)n, 1, device, [&](nl_stack_t *h) {
        const int r = nl_stack_upload_tile(h, 0, data_host);
        return r == NL_OK ? export_gray_impl(h, h->d_frames, min, max, gamma, bits, out_host) : r;
    });
}

// ---- the rgb / lrgb command around its tone curves (internal/fits/rgb.go, pixelops.go:441-550 and :679-692,
// tiff16.go:45-91, writejpg.go:43-89; kernels and host scalars in colour.hip).  The planes are three slots of h. -------

// the three planes named by planes[3]; the thread's error names `who`
static int rgb_planes(nl_stack_t *h, const int *planes, const char *who, nl::Planes *pl)
{
    if (!planes) return fail(NL_ERR_INVALID_ARG, "%s: null planes", who);
    for (int c = 0; c < 3; c++) {
        if (!(pl->p[c] = frame_or_fail(h, planes[c], who))) return NL_ERR_INVALID_ARG;
        for (int k = 0; k < c; k++)
            if (planes[k] == planes[c])
                return fail(NL_ERR_INVALID_ARG, "%s: slot %d names two planes", who, planes[c]);
    }
    return NL_OK;
}

// what every resident colour entry does first (without a device a null handle is NL_ERR_NO_DEVICE)
#define NL_RGB_ENTRY(h, planes, who, pl)                                \
    do {                                                                \
        int rc_ = nl::require_device();                                 \
        if (rc_ != NL_OK) return rc_;                                   \
        NL_CHECK_HANDLE(h);                                             \
        NL_SETTLE_UPLOADS(h);                                           \
        if ((rc_ = rgb_planes(h, planes, who, &pl)) != NL_OK) return rc_; \
    } while (0)

int nl_rgb_normalization(const float mins[3], const float maxs[3], float *min, float *mult)
{
    if (!mins || !maxs || !min || !mult) return fail(NL_ERR_INVALID_ARG, "rgb_normalization: null argument");
    nl::rgb_normalization(mins, maxs, min, mult);
    return NL_OK;
}

int nl_rgb_balance_coeffs(nl_rgb_t cur_shadows, nl_rgb_t cur_highlights, nl_rgb_t target_shadows,
                          nl_rgb_t target_highlights, float alpha[3], float beta[3])
{
    if (!alpha || !beta) return fail(NL_ERR_INVALID_ARG, "rgb_balance_coeffs: null output");
    nl::rgb_balance_coeffs(cur_shadows, cur_highlights, target_shadows, target_highlights, alpha, beta);
    return NL_OK;
}

int nl_stack_frame_combine_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, float min, float mult)
{
    int rc = nl::require_device();
    if (rc != NL_OK) return rc;
    NL_CHECK_HANDLE(src);
    NL_CHECK_HANDLE(dst);
    if (src->device != dst->device)
        return fail(NL_ERR_INVALID_ARG, "frame_combine_from: source on device %d, destination on device %d", src->device,
                    dst->device);
    if (src_idx >= 0) NL_SETTLE_UPLOADS(src);
    NL_SETTLE_UPLOADS(dst);
    if (src_idx < -1) return fail(NL_ERR_INVALID_ARG, "frame_combine_from (source): bad index %d", src_idx);
    const float *s = resident_pixels(src, src_idx, "frame_combine_from (source)", &rc);
    if (!s) return rc;
    float *d = frame_or_fail(dst, dst_idx, "frame_combine_from (destination)");
    if (!d) return NL_ERR_INVALID_ARG;
    if (src->width != dst->width || src->height != dst->height || src->row0 != dst->row0 || src->rows != dst->rows)
        return fail(NL_ERR_INVALID_ARG, "frame_combine_from: source %dx%d rows [%d, %d), destination %dx%d rows [%d, %d)",
                    src->width, src->height, src->row0, src->row0 + src->rows, dst->width, dst->height, dst->row0,
                    dst->row0 + dst->rows);
    if (src != dst && (rc = nl_stack_order_stream_after(src, dst->stream)) != NL_OK) return rc;
    NL_HIP(nl::launch_combine(d, s, dst->npix, min, mult, dst->stream));
    NL_HIP(hipStreamSynchronize(dst->stream));                 // the caller may overwrite the source at once
    return NL_OK;
}

// ScaleOffsetClampRGB on the planes; stats (9 floats or nullptr): {min, mean, max} per plane from the same pass
static int rgb_clamp_impl(nl_stack_t *h, const nl::Planes &pl, const float alpha[3], const float beta[3], float *stats)
{
    if (!stats) {
        NL_HIP(nl::launch_rgb_clamp(pl, h->npix, alpha, beta, nullptr, nullptr, 0, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
        return NL_OK;
    }
    nl::DevBuffer &work = h->frame_scratch.colour_work.stats;
    const size_t part_bytes = sizeof(double) * 3 * kStatBlocks;
    NL_HIP(work.reserve(3 * part_bytes + 3 * sizeof(float), h->stream));
    double *part = static_cast<double *>(work.ptr);
    float *seed = reinterpret_cast<float *>(part + 9 * kStatBlocks);
    NL_HIP(nl::launch_rgb_clamp(pl, h->npix, alpha, beta, seed, part, kStatBlocks, h->stream));
    for (int c = 0; c < 3; c++) {
        const int rc = min_mean_max_from_partials(h, h->npix, stats + 3 * c, stats + 3 * c + 1, stats + 3 * c + 2,
                                                  part + 3 * kStatBlocks * c);
        if (rc != NL_OK) return rc;
    }
    return NL_OK;
}

int nl_stack_rgb_scale_offset_clamp(nl_stack_t *h, const int planes[3], const float alpha[3], const float beta[3],
                                    float stats_out[9])
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_scale_offset_clamp", pl);
    if (!alpha || !beta) return fail(NL_ERR_INVALID_ARG, "rgb_scale_offset_clamp: null coefficients");
    return rgb_clamp_impl(h, pl, alpha, beta, stats_out);
}

// what findDarkestBlock needs of its arguments, and its block grid
static int rgb_darkest_block_check(nl_stack_t *h, const char *who, int block, float border, nl::BlockGrid *g)
{
    if (block < 1) return fail(NL_ERR_INVALID_ARG, "%s: block size %d (findDarkestBlock, rgb.go:158, divides by it)", who, block);
    if (border >= 0.0f) *g = nl::darkest_block_grid(h->width, h->height, block, border);
    if (!(border >= 0.0f) || g->x_first < 0 || g->y_first < 0)
        return fail(NL_ERR_INVALID_ARG, "%s: border %g (rgb.go:158-161: the first block would lie below 0)", who, border);
    int rc = need_whole_image(h, who, "the blocks span rows");
    if (rc == NL_OK) rc = need_int32_pixels(h->npix, who);
    return rc;
}

static int rgb_darkest_block_impl(nl_stack_t *h, const nl::Planes &pl, const char *who, int block, float border,
                                  nl_rgb_t *out)
{
    if (!out) return fail(NL_ERR_INVALID_ARG, "%s: null output", who);
    nl::BlockGrid g;
    const int rc = rgb_darkest_block_check(h, who, block, border, &g);
    if (rc != NL_OK) return rc;
    const int64_t n_blocks = (int64_t)g.nbx * g.nby;
    std::vector<float> means((size_t)(3 * n_blocks));
    if (n_blocks > 0) {
        nl::DevBuffer &work = h->frame_scratch.colour_work.means;
        NL_HIP(work.reserve(sizeof(float) * means.size(), h->stream));
        NL_HIP(nl::launch_block_means(pl, h->width, g, block, (h->dev_flags & kDevColourDirect) != 0,
                                      static_cast<float *>(work.ptr), h->stream));
        NL_HIP(hipMemcpyAsync(means.data(), work.ptr, sizeof(float) * means.size(), hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    *out = nl::darkest_block_scan(means.data(), n_blocks);
    return NL_OK;
}

int nl_stack_rgb_darkest_block(nl_stack_t *h, const int planes[3], int block, float border, nl_rgb_t *out)
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_darkest_block", pl);
    return rgb_darkest_block_impl(h, pl, "rgb_darkest_block", block, border, out);
}

// the stars meanStarIntensity sums: [*first, *first + *n) of the list (*n == 0: the result is {0, 0, 0})
static int rgb_star_selection(nl_stack_t *h, const char *who, const nl_star_t *stars, int n_stars, float skip_bright,
                              float skip_dim, int64_t *first, int *n)
{
    *n = 0;
    if (n_stars < 0 || (n_stars > 0 && !stars)) return fail(NL_ERR_INVALID_ARG, "%s: %d stars", who, n_stars);
    int rc = need_whole_image(h, who, "a star's disc spans rows");
    if (rc == NL_OK) rc = need_int32_pixels(h->npix, who);
    if (rc != NL_OK) return rc;
    if (n_stars == 0) return NL_OK;                            // rgb.go:224
    int64_t s_end;
    nl::star_range(n_stars, skip_bright, skip_dim, first, &s_end);
    if (*first >= s_end) return NL_OK;                         // :228
    if (*first < 0 || s_end > n_stars)                         // (the reference's slice would be out of range)
        return fail(NL_ERR_INVALID_ARG, "%s: skip_bright %g, skip_dim %g select stars [%lld, %lld) of %d (rgb.go:237)",
                    who, skip_bright, skip_dim, (long long)*first, (long long)s_end, n_stars);
    for (int64_t i = *first; i < s_end; i++) {
        const int32_t hfr_r = nl::star_hfr_radius(stars[i].hfr);
        if (!(stars[i].hfr >= 0.0f) || hfr_r < 0 || hfr_r > 1024)
            return fail(NL_ERR_INVALID_ARG, "%s: star %lld has HFR %g (meanStarIntensity, rgb.go:239-240: a disc radius in [0, 1024])",
                        who, (long long)i, stars[i].hfr);
    }
    *n = (int)(s_end - *first);
    return NL_OK;
}

static int rgb_star_intensity_impl(nl_stack_t *h, const nl::Planes &pl, const char *who, const nl_star_t *stars,
                                   int n_stars, float skip_bright, float skip_dim, nl_rgb_t clip, nl_rgb_t *out)
{
    if (!out) return fail(NL_ERR_INVALID_ARG, "%s: null output", who);
    int64_t s_start = 0;
    int n = 0;
    const int rc = rgb_star_selection(h, who, stars, n_stars, skip_bright, skip_dim, &s_start, &n);
    if (rc != NL_OK) return rc;
    *out = nl_rgb_t{0.0f, 0.0f, 0.0f};
    if (n == 0) return NL_OK;
    const nl_star_t *sel = stars + s_start;
    nl::DevBuffer &work = h->frame_scratch.colour_work.stars;
    nl::Carver measure(nullptr);
    measure.take<nl_star_t>((size_t)n);
    measure.take<nl::StarSum>((size_t)n);
    NL_HIP(work.reserve(measure.bytes(), h->stream));
    nl::Carver cv(work.ptr);
    nl_star_t *d_stars = cv.take<nl_star_t>((size_t)n);
    nl::StarSum *d_sums = cv.take<nl::StarSum>((size_t)n);
    std::vector<nl::StarSum> sums((size_t)n);
    NL_HIP(hipMemcpyAsync(d_stars, sel, sizeof(nl_star_t) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    NL_HIP(nl::launch_star_sums(pl, h->width, h->height, d_stars, n, clip, d_sums, h->stream));
    NL_HIP(hipMemcpyAsync(sums.data(), d_sums, sizeof(nl::StarSum) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    *out = nl::star_mean(sums.data(), n);
    return NL_OK;
}

int nl_stack_rgb_mean_star_intensity(nl_stack_t *h, const int planes[3], const nl_star_t *stars, int n_stars,
                                     float skip_bright, float skip_dim, nl_rgb_t clip, nl_rgb_t *out)
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_mean_star_intensity", pl);
    return rgb_star_intensity_impl(h, pl, "rgb_mean_star_intensity", stars, n_stars, skip_bright, skip_dim, clip, out);
}

// SetBlackWhitePoints (rgb.go:94-120) on the planes
static int rgb_balance_impl(nl_stack_t *h, const nl::Planes &pl, const char *who, const nl_star_t *stars, int n_stars,
                            int block, float border, float skip_bright, float skip_dim, nl_rgb_t shadows,
                            nl_rgb_t highlights, const float loc[3], const float scale[3], nl_rgb_balance_t *report)
{
    if (!loc || !scale) return fail(NL_ERR_INVALID_ARG, "%s: null location or scale", who);
    nl::BlockGrid grid;                                    // every argument is checked before the first pass writes
    int64_t first;
    int n_selected;
    int rc = rgb_darkest_block_check(h, who, block, border, &grid);
    if (rc == NL_OK) rc = rgb_star_selection(h, who, stars, n_stars, skip_bright, skip_dim, &first, &n_selected);
    if (rc != NL_OK) return rc;
    nl_rgb_balance_t rep;
    const nl_rgb_t location{loc[0], loc[1], loc[2]};
    const nl_rgb_t scaled{loc[0] + scale[0] * 3.0f, loc[1] + scale[1] * 3.0f, loc[2] + scale[2] * 3.0f};      // :101
    nl::rgb_balance_coeffs(location, scaled, shadows, highlights, rep.alpha1, rep.beta1);
    float stats[9];
    if ((rc = rgb_clamp_impl(h, pl, rep.alpha1, rep.beta1, stats)) != NL_OK) return rc;
    if ((rc = rgb_darkest_block_impl(h, pl, who, block, border, &rep.darkest)) != NL_OK) return rc;
    const float clip = 0.9f;                                                                                   // :113
    const nl_rgb_t clips{stats[2] * clip, stats[5] * clip, stats[8] * clip};
    if ((rc = rgb_star_intensity_impl(h, pl, who, stars, n_stars, skip_bright, skip_dim, clips, &rep.stars)) != NL_OK)
        return rc;
    nl::rgb_balance_coeffs(rep.darkest, rep.stars, shadows, highlights, rep.alpha2, rep.beta2);
    if ((rc = rgb_clamp_impl(h, pl, rep.alpha2, rep.beta2, nullptr)) != NL_OK) return rc;
    if (report) *report = rep;
    return NL_OK;
}

int nl_stack_rgb_balance(nl_stack_t *h, const int planes[3], const nl_star_t *stars, int n_stars, int block,
                         float border, float skip_bright, float skip_dim, nl_rgb_t shadows, nl_rgb_t highlights,
                         const float loc[3], const float scale[3], nl_rgb_balance_t *report)
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_balance", pl);
    return rgb_balance_impl(h, pl, "rgb_balance", stars, n_stars, block, border, skip_bright, skip_dim, shadows,
                            highlights, loc, scale, report);
}

// three planes of host memory on a handle of the call's own: up, run(h, planes), and with `down` back into the planes
extern "C++" template <class Run>
static int host_planes_run(const float *planar_host, float *planar_out, int width, int height, int device, Run run)
{
    return with_scratch_frames(3, width, height, device, [&](nl_stack_t *h) {
        const size_t n = (size_t)width * (size_t)height;
        int r = NL_OK;
        for (int c = 0; c < 3 && r == NL_OK; c++) r = nl_stack_upload_tile(h, c, planar_host + n * c);
        nl::Planes pl;
        const int planes[3] = {0, 1, 2};
        if (r == NL_OK) r = rgb_planes(h, planes, "host planes", &pl);
        if (r == NL_OK) r = run(h, pl);
        for (int c = 0; c < 3 && r == NL_OK && planar_out; c++) r = nl_stack_download_tile(h, c, planar_out + n * c);
        return r;
    });
}

int nl_rgb_balance(float *planar_host, int width, int height, const nl_star_t *stars, int n_stars, int block,
                   float border, float skip_bright, float skip_dim, nl_rgb_t shadows, nl_rgb_t highlights,
                   const float loc[3], const float scale[3], nl_rgb_balance_t *report, int device)
{
    if (!planar_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "rgb_balance: bad argument");
    const int rc = select_device(device);
    if (rc != NL_OK) return rc;
    return host_planes_run(planar_host, planar_host, width, height, device, [&](nl_stack_t *h, const nl::Planes &pl) {
        return rgb_balance_impl(h, pl, "rgb_balance", stars, n_stars, block, border, skip_bright, skip_dim, shadows,
                                highlights, loc, scale, report);
    });
}

int nl_stack_rgb_chroma(nl_stack_t *h, const int planes[3], const nl_chroma_t *op)
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_chroma", pl);
    if (!op) return fail(NL_ERR_INVALID_ARG, "rgb_chroma: null operation");
    if (!nl::chroma_kind_known(op->kind))
        return fail(NL_ERR_INVALID_ARG, "rgb_chroma: unknown kind %d (NL_CHROMA_GAMMA ... NL_ROTATE_HUES)", op->kind);
    NL_HIP(nl::launch_chroma(pl, h->npix, *op, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// the R G B A counts of the planes into out_host, through the handle's ingest buffer like the gray export
static int export_rgb_impl(nl_stack_t *h, const nl::Planes &pl, float min, float max, float gamma, int bits, void *out_host)
{
    const float scale = 1.0f / (max - min);                    // tiff16.go:50-51
    const double gamma_inv = (double)(1.0f / gamma);
    const size_t bytes = (size_t)h->npix * (size_t)(bits / 2);
    NL_HIP(h->ingest.reserve(bytes, h->stream));
    NL_HIP(nl::launch_export_rgb(pl, h->npix, min, scale, gamma_inv != 1.0, gamma_inv, bits, h->ingest.ptr, h->stream));
    NL_HIP(hipMemcpyAsync(out_host, h->ingest.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl_stack_rgb_export(nl_stack_t *h, const int planes[3], float min, float max, float gamma, int bits, void *out_host)
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_export", pl);
    const int rc = export_gray_check("rgb_export", gamma, bits, out_host);
    return rc == NL_OK ? export_rgb_impl(h, pl, min, max, gamma, bits, out_host) : rc;
}

int nl_export_rgb(const float *planar_host, int64_t n, float min, float max, float gamma, int bits, void *out_host,
                  int device)
{
    if (!planar_host || n < 1 || n > 0x7fffffff) return fail(NL_ERR_INVALID_ARG, "export_rgb: bad argument");
    int rc = export_gray_check("export_rgb", gamma, bits, out_host);
    if (rc == NL_OK) rc = select_device(device);
    if (rc != NL_OK) return rc;
    return host_planes_run(planar_host, nullptr, (int)n, 1, device, [&](nl_stack_t *h, const nl::Planes &pl) {
        return export_rgb_impl(h, pl, min, max, gamma, bits, out_host);
    });
}

// ---- OpAlign's f.Project from a resident frame (post/postprocess.go:185, fits/project.go:26-76; kernel in project.hip) ----

}  // extern "C"

namespace {

// the checks both forms share; *s = the source slot, *d = the destination slot, inv = the inverse transform
int project_from_check(const char *who, nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float *trans,
                       const float **s, float **d, float inv[6])
{
    char part[96];
    snprintf(part, sizeof part, "%s (source)", who);
    *s = frame_or_fail(src, src_idx, part);
    if (!*s) return NL_ERR_INVALID_ARG;
    snprintf(part, sizeof part, "%s (destination)", who);
    *d = frame_or_fail(dst, dst_idx, part);
    if (!*d) return NL_ERR_INVALID_ARG;
    if (!trans) return fail(NL_ERR_INVALID_ARG, "%s: null transform", who);
    snprintf(part, sizeof part, "%s (source)", who);
    int rc = need_whole_image(src, part, "a projection reads any row of the source");
    if (rc == NL_OK) rc = need_int32_pixels(src->npix, who, "source frame");
    if (rc == NL_OK) rc = need_int32_pixels(dst->npix, who, "destination tile");
    if (rc != NL_OK) return rc;
    if (dst->d_frames != dst->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "%s: the destination's frames are attached, not owned", who);
    if (*s == *d) return fail(NL_ERR_INVALID_ARG, "%s: slot %d of one handle is source and destination (a projection cannot run in place)", who, src_idx);
    return invert_transform(trans, inv);
}

// the source rows [*y0, *y1] that the destination rows of dst can tap (project.hpp: the corners of a rectangle bound
// every pixel's coordinates); false: none
bool project_source_rows(const nl_stack_t *dst, const nl_stack_t *src, const float inv[6], int *y0, int *y1)
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
    *y0 = std::max(nl::proj_floor_clamped(lo), 0);
    *y1 = std::min(nl::proj_floor_clamped(hi) + 1, src->height - 1);
    return *y0 <= *y1;
}

}  // namespace

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
                           float out_of_bounds, const char *who, bool from_group)
{
    NL_CHECK_HANDLE(src);
    NL_CHECK_HANDLE(dst);
    if (src->device != dst->device && !from_group)
        return fail(NL_ERR_INVALID_ARG, "%s: source on device %d, destination on device %d", who, src->device, dst->device);
    if (!from_group) NL_SETTLE_UPLOADS(src);
    NL_SETTLE_UPLOADS(dst);
    const float *s = nullptr;
    float *d = nullptr;
    float inv[6];
    int rc = project_from_check(who, dst, dst_idx, src, src_idx, trans, &s, &d, inv);
    if (rc != NL_OK) return rc;
    if (src != dst && !from_group && (rc = nl_stack_order_stream_after(src, dst->stream)) != NL_OK) return rc;
    NL_HIP(hipSetDevice(dst->device));
    if (src->device != dst->device) {
        NL_HIP(dst->ingest.reserve((size_t)src->npix * sizeof(float), dst->stream));
        int y0 = 0, y1 = 0;
        if (project_source_rows(dst, src, inv, &y0, &y1)) {
            const size_t at = (size_t)y0 * (size_t)src->width;
            NL_HIP(hipMemcpyPeerAsync(static_cast<float *>(dst->ingest.ptr) + at, dst->device, s + at, src->device,
                                      sizeof(float) * (size_t)(y1 - y0 + 1) * (size_t)src->width, dst->stream));
        }
        s = static_cast<const float *>(dst->ingest.ptr);
    }
    NL_HIP(nl::launch_project_tiled(s, src->width, src->height, d, dst->width, dst->row0, dst->rows, inv, out_of_bounds,
                                    project_switches(dst), dst->stream));
    NL_HIP(hipStreamSynchronize(dst->stream));                 // the caller may overwrite the source slot at once
    return NL_OK;
}

extern "C" {

int nl_stack_frame_project_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float trans[6],
                                float out_of_bounds)
{
    return nl::stack_project_from(dst, dst_idx, src, src_idx, trans, out_of_bounds, "frame_project_from", false);
}

int nl_stack_project_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], int64_t *staged,
                                int64_t *direct)
{
    if (!dst || !src || !trans || !staged || !direct) return fail(NL_ERR_INVALID_ARG, "project_tile_paths: null argument");
    const float *s = frame_or_fail(src, src_idx, "project_tile_paths");
    if (!s) return NL_ERR_INVALID_ARG;
    float inv[6];
    const int rc = invert_transform(trans, inv);
    if (rc != NL_OK) return rc;
    nl::project_tile_paths(s, src->width, src->height, dst->width, dst->row0, dst->rows, inv, project_switches(dst),
                           staged, direct);
    return NL_OK;
}

int nl_bin_nxn(const float *in_host, int width, int height, int n, float *out_host, int device)
{
    if (!in_host || !out_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "bin_nxn: bad argument");
    int rc = select_device(device);
    if (rc != NL_OK) return rc;
    int ow, oh;
    if ((rc = nl_bin_shape(width, height, n, &ow, &oh)) != NL_OK) return rc;
    if (n <= 1) {
        if (out_host != in_host) memmove(out_host, in_host, sizeof(float) * (size_t)width * height);
        return NL_OK;
    }
    return with_scratch_handle(width, height, device, [&](nl_stack_t *src) {
        const int r = nl_stack_upload_tile(src, 0, in_host);
        if (r != NL_OK) return r;
        return with_scratch_handle(ow, oh, device, [&](nl_stack_t *dst) {
            const int rb = nl_stack_frame_bin_from(dst, 0, src, 0, n);
            return rb == NL_OK ? nl_stack_download_tile(dst, 0, out_host) : rb;
        });
    });
}

// ---- OpBadPixel, Bayer branch, and OpDebayer (internal/ops/pre/preprocess.go:180-251; kernels in bayer.hip) -------

// getOffsets (debayer.go:26-37)
static int cfa_offsets(const char *cfa, int *xo, int *yo)
{
    const std::string c = cfa;
    if (c == "RGGB" || c == "rggb") { *xo = 0; *yo = 0; }
    else if (c == "GRBG" || c == "grbg") { *xo = 1; *yo = 0; }
    else if (c == "GBRG" || c == "gbrg") { *xo = 0; *yo = 1; }
    else if (c == "BGGR" || c == "bggr") { *xo = 1; *yo = 1; }
    else return fail(NL_ERR_INVALID_ARG, "Unknown CFA value %s", cfa);
    return NL_OK;
}

// the channel switch of CosmeticCorrectionBayer / DebayerBilinear (badpixels_bayer.go:36-45, debayer.go:47-59)
static int cfa_channel(const char *channel, int *ch)
{
    const std::string c = channel;
    if (c == "R" || c == "r") *ch = nl::kBayerR;
    else if (c == "G" || c == "g") *ch = nl::kBayerG;
    else if (c == "B" || c == "b") *ch = nl::kBayerB;
    else return fail(NL_ERR_INVALID_ARG, "Unknown debayering value %s", channel);
    return NL_OK;
}

// the CFA, then the channel, as the reference checks them; the output shape of DebayerBilinear (debayer.go:65-66)
static int cfa_parse(const char *channel, const char *cfa, int width, int height, int *ch, int *xo, int *yo,
                     int *out_w, int *out_h)
{
    int rc = cfa_offsets(cfa, xo, yo);
    if (rc == NL_OK) rc = cfa_channel(channel, ch);
    if (rc != NL_OK) return rc;
    *out_w = (width - *xo) & ~1;
    *out_h = (height - *yo) & ~1;
    if ((int64_t)*out_w * *out_h == 0)        // (the reference divides by the width 0 at preprocess.go:245)
        return fail(NL_ERR_INVALID_ARG, "debayer: %dx%d mosaic with cfa %s gives an empty %dx%d image", width, height,
                    cfa, *out_w, *out_h);
    return NL_OK;
}

int nl_debayer_shape(int width, int height, const char *channel, const char *cfa, int *out_width, int *out_height)
{
    if (width < 1 || height < 1 || !out_width || !out_height)
        return fail(NL_ERR_INVALID_ARG, "debayer_shape: bad argument");
    if (!channel || !cfa || !*channel || !*cfa) {            // OpDebayer.Apply is a no-op (preprocess.go:240-242)
        *out_width = width;
        *out_height = height;
        return NL_OK;
    }
    int ch, xo, yo;
    return cfa_parse(channel, cfa, width, height, &ch, &xo, &yo, out_width, out_height);
}

int nl_stack_upload_frame_cfa(nl_stack_t *h, int idx, const float *raw_host, int raw_width, int raw_height,
                              const nl_calib_t *c, const char *channel, const char *cfa, float sigma_low,
                              float sigma_high, int64_t *removed_out, float *stats_out)
{
    int rc = nl::require_device();            // (before the handle: without a device a null handle is NL_ERR_NO_DEVICE)
    if (rc != NL_OK) return rc;
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    if (idx < 0 || idx >= h->n_frames || !raw_host || raw_width < 1 || raw_height < 1)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_cfa: bad index %d, null frame or bad raw size %dx%d", idx,
                    raw_width, raw_height);
    if (!channel || !cfa || !*channel || !*cfa)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_cfa needs a channel and a CFA (mono frames: nl_stack_upload_tile, "
                    "nl_stack_frame_calibrate, nl_stack_frame_badpixel)");
    int ch, xo, yo, out_w, out_h;
    if ((rc = cfa_parse(channel, cfa, raw_width, raw_height, &ch, &xo, &yo, &out_w, &out_h)) != NL_OK) return rc;
    if ((rc = need_whole_image(h, "upload_frame_cfa", "3x3 stencil, whole-frame std")) != NL_OK) return rc;
    if (h->width != out_w || h->height != out_h)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_cfa: a %dx%d mosaic debayers to %dx%d, the handle is %dx%d",
                    raw_width, raw_height, out_w, out_h, h->width, h->height);
    const int64_t n = (int64_t)raw_width * raw_height;
    if ((rc = need_int32_pixels(n, "upload_frame_cfa", "mosaic")) != NL_OK) return rc;
    if (c) {
        if (c->device != h->device)
            return fail(NL_ERR_INVALID_ARG, "upload_frame_cfa: calibration on device %d, handle on device %d",
                        c->device, h->device);
        if ((rc = calib_check_light(c, idx, raw_width, raw_height)) != NL_OK) return rc;
    }
    const nl::BayerGeom g = nl::bayer_geom(raw_width, raw_height, ch, xo, yo);
    float *raw;
    nl::BayerScratch s;
    auto carve = [&](void *base) {
        nl::Carver cv(base);
        raw = cv.take<float>((size_t)n);
        s.delta = cv.take<float>((size_t)g.rows * g.cstride);
        s.median = cv.take<float>((size_t)g.rows * g.cstride);
        s.rowsum = cv.take<float>((size_t)g.rows);
        s.removed = cv.take<unsigned>((size_t)nl::bayer_replace_blocks(g));
        s.params = cv.take<nl::BayerParams>(1);
        return cv.bytes();
    };
    NL_HIP(h->frame_scratch.cfa.reserve(carve(nullptr), h->stream));
    carve(h->frame_scratch.cfa.ptr);
    NL_HIP(hipMemcpyAsync(raw, raw_host, sizeof(float) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    if (c)
        NL_HIP(nl::launch_calibrate(raw, raw, n, c->d_dark, c->d_flat, c->flat_max, h->stream));
    const bool correct = sigma_low != 0.0f && sigma_high != 0.0f;     // preprocess.go:181-183
    if (correct) NL_HIP(nl::launch_bayer_correct(raw, g, sigma_low, sigma_high, s, h->stream));
    NL_HIP(nl::launch_debayer(raw, raw_width, raw_height, ch, xo, yo, h->d_frames + (int64_t)idx * h->fstride,
                              h->width, h->stream));
    nl::BayerParams p;
    p.mean = p.std = NAN;
    p.removed = 0;
    if (correct) NL_HIP(hipMemcpyAsync(&p, s.params, sizeof p, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));   // (raw_host must not be retained)
    if (removed_out) *removed_out = (int64_t)p.removed;
    if (stats_out) { stats_out[0] = p.mean; stats_out[1] = p.std; }
    return NL_OK;
}

int nl_preprocess_frame_cfa(const nl_calib_t *c, int frame_id, const float *in_host, int width, int height,
                            const char *channel, const char *cfa, float sigma_low, float sigma_high, float *out_host,
                            int *out_width, int *out_height, int64_t *removed_out, float *stats_out, int device)
{
    int rc = preprocess_check("preprocess_frame_cfa", c, frame_id, in_host, out_host, width, height, device);
    if (rc != NL_OK) return rc;                                 // (OpCalibrate first)
    const char *chan = channel ? channel : "", *pattern = cfa ? cfa : "";
    const bool correct = sigma_low != 0.0f && sigma_high != 0.0f;
    int ch, xo, yo, ow = width, oh = height;
    if (*chan && correct && (rc = cfa_parse(chan, pattern, width, height, &ch, &xo, &yo, &ow, &oh)) != NL_OK)
        return rc;                                              // OpBadPixel's Bayer branch: CFA, then channel
    if (!*chan || !*pattern) {
        // the mono branch of OpBadPixel (or none) and no OpDebayer: nl_preprocess_frame's result
        if (out_width) *out_width = width;
        if (out_height) *out_height = height;
        return nl_preprocess_frame(c, frame_id, in_host, out_host, width, height, *chan ? 0.0f : sigma_low,
                                   *chan ? 0.0f : sigma_high, removed_out, stats_out, device);
    }
    if ((rc = cfa_parse(chan, pattern, width, height, &ch, &xo, &yo, &ow, &oh)) != NL_OK) return rc;   // OpDebayer
    // (a handle of the debayered shape)
    rc = with_scratch_handle(ow, oh, device, [&](nl_stack_t *h) {
        const int r = nl_stack_upload_frame_cfa(h, 0, in_host, width, height, c, chan, pattern, sigma_low, sigma_high,
                                                removed_out, stats_out);
        return r == NL_OK ? nl_stack_download_tile(h, 0, out_host) : r;
    });
    if (rc == NL_OK) {
        if (out_width) *out_width = ow;
        if (out_height) *out_height = oh;
    }
    return rc;
}

}  // extern "C"
