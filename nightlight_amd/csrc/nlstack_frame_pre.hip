// nlstack_frame_pre.hip -- the preprocessing operators on one frame resident in a handle, and their host forms:
// OpCalibrate and OpBadPixel (internal/ops/pre/preprocess.go:68-195), the colour-camera front (OpBadPixel's Bayer
// branch and OpDebayer, preprocess.go:180-251, debayer.go), OpStarDetect (internal/star/findstars.go:59-103),
// OpBackExtract (ops/pre/background.go:68-462), OpDebandHoriz / OpDebandVert (ops/pre/banding.go:61-270) and OpBin
// (preprocess.go:324-331, internal/fits/fits.go:163-195).  Kernels in preprocess.hip, bayer.hip, stars.hip,
// background.hip and deband.hip; the flat's maximum through frame_stats.hip.
#include <float.h>
#include <math.h>

#include <algorithm>

#include "bayer.hpp"
#include "preprocess.hpp"
#include "nlstack_frame_common.hpp"

extern "C" {

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
    *out = nl::fold_min_sum_max(part).hi;
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
    float *d;
    if (const int rc = resident_entry(h, idx, "frame_badpixel", false, &d); rc != NL_OK) return rc;
    if (sigma_low == 0.0f || sigma_high == 0.0f) {         // preprocess.go:181-183: nothing to do
        if (removed_out) *removed_out = 0;
        if (diff_stats_out) diff_stats_out[0] = diff_stats_out[1] = NAN;
        return NL_OK;
    }
    if (sigma_low < 0.0f || sigma_high < 0.0f)             // (the reference would flag the border: not supported)
        return fail(NL_ERR_INVALID_ARG, "frame_badpixel: negative sigma (low %g, high %g)", sigma_low, sigma_high);
    if (const int rc = need_whole_frame(h, "frame_badpixel", "3x3 stencil, whole-frame std"); rc != NL_OK) return rc;
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
    if (const int rc = select_device(device); rc != NL_OK) return rc;
    if (c && c->device != device)
        return fail(NL_ERR_INVALID_ARG, "%s: calibration on device %d, frame on device %d", who, c->device, device);
    return c ? calib_check_light(c, frame_id, width, height) : NL_OK;
}

int nl_preprocess_frame(const nl_calib_t *c, int frame_id, const float *in_host, float *out_host, int width, int height,
                        float sigma_low, float sigma_high, int64_t *removed_out, float *diff_stats_out, int device)
{
    const int rc = preprocess_check("preprocess_frame", c, frame_id, in_host, out_host, width, height, device);
    if (rc != NL_OK) return rc;
    return host_frames_run(1, in_host, out_host, width, height, device, [&](nl_stack_t *h) {
        const int r = c ? nl_stack_frame_calibrate(h, 0, c) : NL_OK;
        return r == NL_OK ? nl_stack_frame_badpixel(h, 0, sigma_low, sigma_high, removed_out, diff_stats_out) : r;
    });
}

// ---- OpBadPixel, Bayer branch, and OpDebayer (internal/ops/pre/preprocess.go:180-251; kernels in bayer.hip) -------

// the names (cfa_names of nlstack_frame_common.hpp), then the output shape of DebayerBilinear (debayer.go:65-66)
static int cfa_parse(const char *channel, const char *cfa, int width, int height, int *ch, int *xo, int *yo,
                     int *out_w, int *out_h)
{
    if (const int rc = cfa_names(channel, cfa, ch, xo, yo); rc != NL_OK) return rc;
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

// ---- OpStarDetect: star.FindStars (internal/star/findstars.go:59-103; kernels and host steps in stars.hip) ---------

static int find_stars_impl(nl_stack_t *h, const float *d_data, const char *who, const nl::StarParams &p,
                           nl_star_t *stars_out, int capacity, int *n_stars, float *sum_of_shifts, float *avg_hfr)
{
    if (p.radius < 0 || p.radius > 1024)      // (deviation 2; radius 0 finds no star)
        return fail(NL_ERR_INVALID_ARG, "%s: radius %d not in [0, 1024]", who, p.radius);
    int pre = check_capacity(who, capacity, stars_out);
    if (pre == NL_OK) pre = need_whole_frame(h, who, "FindStars indexes the data 1-D");
    if (pre != NL_OK) return pre;
    if (!h->d_stat_partial) NL_HIP(dev_malloc(&h->d_stat_partial, sizeof(double) * 3 * kStatBlocks));
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
    float *d;
    if (const int rc = resident_entry(h, idx, "frame_find_stars", false, &d); rc != NL_OK) return rc;
    const nl::StarParams p{location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std};
    return find_stars_impl(h, d, "frame_find_stars", p, stars_out, capacity, n_stars, sum_of_shifts, avg_hfr);
}

int nl_stack_result_find_stars(nl_stack_t *h, float location, float scale, float star_sig, float bp_sigma,
                               float star_in_out, int radius, float diff_std, nl_star_t *stars_out, int capacity,
                               int *n_stars, float *sum_of_shifts, float *avg_hfr)
{
    float *d;
    if (const int rc = resident_entry(h, -1, "result_find_stars", true, &d); rc != NL_OK) return rc;
    const nl::StarParams p{location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std};
    return find_stars_impl(h, d, "result_find_stars", p, stars_out, capacity, n_stars, sum_of_shifts, avg_hfr);
}

int nl_find_stars(const float *data_host, int width, int height, float location, float scale, float star_sig,
                  float bp_sigma, float star_in_out, int radius, float diff_std, nl_star_t *stars_out, int capacity,
                  int *n_stars, float *sum_of_shifts, float *avg_hfr, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "find_stars: bad argument");
    if (const int rc = select_device(device); rc != NL_OK) return rc;
    const nl::StarParams p{location, scale, star_sig, bp_sigma, star_in_out, radius, diff_std};
    return host_frames_run(1, data_host, nullptr, width, height, device, [&](nl_stack_t *h) {
        return find_stars_impl(h, h->d_frames, "find_stars", p, stars_out, capacity, n_stars, sum_of_shifts, avg_hfr);
    });
}

// ---- OpBackExtract: pre.NewBackground + Subtract / Render (internal/ops/pre/background.go:68-462; background.hip) --

static int back_extract_impl(nl_stack_t *h, float *d_data, const char *who, int grid_size, float hfr_factor,
                             float sigma, int clip, const nl_star_t *stars, int n_stars, float *background_out,
                             float *cells_out, int cells_capacity, nl_background_t *info)
{
    int pre = check_stars(who, stars, n_stars);
    if (pre == NL_OK) pre = check_capacity(who, cells_capacity, cells_out);
    if (pre == NL_OK) pre = need_whole_frame(h, who, "the grid spans the whole frame");
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
    float *d;
    if (const int rc = resident_entry(h, idx, "frame_back_extract", false, &d); rc != NL_OK) return rc;
    return back_extract_impl(h, d, "frame_back_extract", grid_size, hfr_factor, sigma, clip, stars, n_stars,
                             background_out, cells_out, cells_capacity, info);
}

int nl_back_extract(float *data_host, int width, int height, int grid_size, float hfr_factor, float sigma, int clip,
                    const nl_star_t *stars, int n_stars, float *background_out, float *cells_out, int cells_capacity,
                    nl_background_t *info, int device)
{
    if (!data_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "back_extract: bad argument");
    if (const int rc = select_device(device); rc != NL_OK) return rc;
    auto run = [&](nl_stack_t *h) {
        return back_extract_impl(h, h->d_frames, "back_extract", grid_size, hfr_factor, sigma, clip, stars, n_stars,
                                 background_out, cells_out, cells_capacity, info);
    };
    if (grid_size <= 0) return with_scratch_handle(1, 1, device, run);     // no-op: the frame is not even uploaded
    return host_frames_run(1, data_host, data_host, width, height, device, run);
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
    const int pre = need_whole_frame(h, who, "the window needs every row's percentile");
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
    float *d;
    const int rc = resident_entry(h, idx, who, false, &d);
    return rc == NL_OK ? deband_impl(h, d, who, cols, percentile, window, sigma, location, scale, info) : rc;
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
    if (const int rc = select_device(device); rc != NL_OK) return rc;
    auto run = [&](nl_stack_t *h) {
        return deband_impl(h, h->d_frames, who, cols, percentile, window, sigma, location, scale, info);
    };
    if (deband_is_noop(cols, percentile, window)) return with_scratch_handle(1, 1, device, run);     // (not even uploaded)
    return host_frames_run(1, data_host, data_host, width, height, device, run);
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
    float *s, *d;
    int rc = resident_target(src, src_idx, "frame_bin_from (source)", false, &s);
    if (rc == NL_OK) rc = resident_target(dst, dst_idx, "frame_bin_from (destination)", false, &d);
    if (rc != NL_OK) return rc;
    rc = need_whole_image(src, "frame_bin_from (source)", "a bin spans rows");
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
    return host_frames_run(1, in_host, nullptr, width, height, device, [&](nl_stack_t *src) {
        return with_scratch_handle(ow, oh, device, [&](nl_stack_t *dst) {
            const int rb = nl_stack_frame_bin_from(dst, 0, src, 0, n);
            return rb == NL_OK ? nl_stack_download_tile(dst, 0, out_host) : rb;
        });
    });
}

}  // extern "C"
