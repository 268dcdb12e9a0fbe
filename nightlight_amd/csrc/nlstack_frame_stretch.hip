// nlstack_frame_stretch.hip -- the stretch command on one frame or result resident in a handle, and its host forms:
// OpGaussianBlur / OpUnsharpMask (internal/ops/stretch/stretch.go:339-424, usm.go), the tone curves
// (stretch.go:40-335, internal/fits/pixelops.go) and OpSave's gray quantisation (tiff16.go, writejpg.go).  Kernels in
// blur.hip and tone.hip.
#include "nlstack_frame_common.hpp"

extern "C" {

// ---- OpGaussianBlur / OpUnsharpMask (internal/ops/stretch/stretch.go:339-424, usm.go; kernels in blur.hip) ---------

int nl_gaussian_kernel_1d(float sigma, float *taps_out, int capacity, int *n_taps_out)
{
    int rc = check_capacity("gaussian_kernel_1d", capacity, taps_out);
    if (rc != NL_OK) return rc;
    std::vector<float> taps;
    std::string msg;
    rc = nl::gaussian_kernel_1d(sigma, taps, &msg);
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
    int pre = need_whole_frame(h, who, "the column pass needs every row");
    if (pre == NL_OK) pre = blur_check_taps(who, taps, n_taps, h->width, h->height);
    if (pre != NL_OK) return pre;
    std::string msg;
    const int rc = nl::blur_run(d_data, h->width, h->height, taps, n_taps, usm, h->frame_scratch.blur_work, h->stream, &msg);
    return rc == NL_OK ? NL_OK : fail(rc, "%s: %s", who, msg.c_str());
}

// the resident sigma forms, on resident_target(h, idx, who, result_ok)
static int resident_blur(nl_stack_t *h, int idx, bool result_ok, const char *who, float sigma, const nl::UsmParams *usm)
{
    float *d;
    if (const int rc = resident_entry(h, idx, who, result_ok, &d); rc != NL_OK) return rc;
    std::vector<float> taps;
    bool noop;
    const int rc = blur_taps(who, sigma, usm, taps, &noop);
    if (rc != NL_OK || noop) return rc;
    return blur_impl(h, d, who, taps.data(), (int)taps.size(), usm);
}

int nl_stack_frame_gaussian_blur(nl_stack_t *h, int idx, float sigma)
{
    return resident_blur(h, idx, false, "frame_gaussian_blur", sigma, nullptr);
}

int nl_stack_frame_unsharp_mask(nl_stack_t *h, int idx, float sigma, float gain, float min, float max,
                                float abs_threshold)
{
    const nl::UsmParams p{gain, min, max, abs_threshold};
    return resident_blur(h, idx, false, "frame_unsharp_mask", sigma, &p);
}

int nl_stack_result_gaussian_blur(nl_stack_t *h, float sigma)
{
    return resident_blur(h, -1, true, "result_gaussian_blur", sigma, nullptr);
}

int nl_stack_result_unsharp_mask(nl_stack_t *h, float sigma, float gain, float min, float max, float abs_threshold)
{
    const nl::UsmParams p{gain, min, max, abs_threshold};
    return resident_blur(h, -1, true, "result_unsharp_mask", sigma, &p);
}

// the host forms: the frame up, the two passes on a handle of the call's own, the frame down into out_host
static int host_blur(const char *who, const float *in_host, float *out_host, int width, int height, const float *taps,
                     int n_taps, const nl::UsmParams *usm, int device)
{
    int rc = blur_check_taps(who, taps, n_taps, width, height);
    if (rc == NL_OK) rc = select_device(device);
    if (rc != NL_OK) return rc;
    return host_frames_run(1, in_host, out_host, width, height, device, [&](nl_stack_t *h) {
        return blur_impl(h, h->d_frames, who, taps, n_taps, usm);
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
static int tone_impl(nl_stack_t *h, float *d, const nl::ToneArgs &args, bool noop, float *mn, float *mean, float *mx)
{
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

// what needs no device: the curve's kind and arguments (and *noop: the operator's own guard holds)
static int tone_check(const char *who, const nl_tone_t *tone, nl::ToneArgs *args, bool *noop)
{
    if (!tone) return fail(NL_ERR_INVALID_ARG, "%s: null curve", who);
    std::string msg;
    const int rc = nl::tone_args(*tone, args, noop, &msg);
    return rc == NL_OK ? NL_OK : fail(rc, "%s: %s", who, msg.c_str());
}

// the resident forms: the call's own arguments, then resident_target(h, idx, who, result_ok)
static int resident_tone(nl_stack_t *h, int idx, bool result_ok, const char *who, const nl_tone_t *tone, float *mn,
                         float *mean, float *mx)
{
    NL_CHECK_HANDLE(h);
    nl::ToneArgs args;
    bool noop;
    float *d;
    int rc = tone_check(who, tone, &args, &noop);
    if (rc == NL_OK) rc = resident_target(h, idx, who, result_ok, &d);
    return rc == NL_OK ? tone_impl(h, d, args, noop, mn, mean, mx) : rc;
}

static int resident_export_gray(nl_stack_t *h, int idx, bool result_ok, const char *who, float min, float max,
                                float gamma, int bits, void *out_host)
{
    NL_CHECK_HANDLE(h);
    float *d;
    int rc = export_check(who, gamma, bits, out_host);
    if (rc == NL_OK) rc = resident_target(h, idx, who, result_ok, &d);
    return rc == NL_OK ? export_impl(h, d, nullptr, min, max, gamma, bits, out_host) : rc;
}

int nl_stack_frame_tone(nl_stack_t *h, int idx, const nl_tone_t *tone, float *mn, float *mean, float *mx)
{
    return resident_tone(h, idx, false, "frame_tone", tone, mn, mean, mx);
}

int nl_stack_result_tone(nl_stack_t *h, const nl_tone_t *tone, float *mn, float *mean, float *mx)
{
    return resident_tone(h, -1, true, "result_tone", tone, mn, mean, mx);
}

int nl_stack_frame_export_gray(nl_stack_t *h, int idx, float min, float max, float gamma, int bits, void *out_host)
{
    return resident_export_gray(h, idx, false, "frame_export_gray", min, max, gamma, bits, out_host);
}

int nl_stack_result_export_gray(nl_stack_t *h, float min, float max, float gamma, int bits, void *out_host)
{
    return resident_export_gray(h, -1, true, "result_export_gray", min, max, gamma, bits, out_host);
}

// the host forms: n floats as an n x 1 frame of a handle of the call's own (like nl_fits_decode)
int nl_tone(float *data_host, int64_t n, const nl_tone_t *tone, float *mn, float *mean, float *mx, int device)
{
    if (!data_host || n < 1 || n > 0x7fffffff) return fail(NL_ERR_INVALID_ARG, "tone: bad argument");
    nl::ToneArgs args;
    bool noop;
    int rc = tone_check("tone", tone, &args, &noop);
    if (rc != NL_OK) return rc;
    if (noop && !mn && !mean && !mx) return NL_OK;             // nothing to compute: the frame is not even uploaded
    if ((rc = select_device(device)) != NL_OK) return rc;
    return host_frames_run(1, data_host, data_host, (int)n, 1, device, [&](nl_stack_t *h) {
        return tone_impl(h, h->d_frames, args, noop, mn, mean, mx);
    });
}

int nl_export_gray(const float *data_host, int64_t n, float min, float max, float gamma, int bits, void *out_host,
                   int device)
{
    if (!data_host || n < 1 || n > 0x7fffffff) return fail(NL_ERR_INVALID_ARG, "export_gray: bad argument");
    int rc = export_check("export_gray", gamma, bits, out_host);
    if (rc == NL_OK) rc = select_device(device);
    if (rc != NL_OK) return rc;
    return host_frames_run(1, data_host, nullptr, (int)n, 1, device, [&](nl_stack_t *h) {
        return export_impl(h, h->d_frames, nullptr, min, max, gamma, bits, out_host);
    });
}

}  // extern "C"
