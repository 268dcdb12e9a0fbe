// nlstack_frame_rgb.hip -- the rgb / lrgb command around its tone curves, on three slots of one handle, and its host
// forms: NewRGBFromChannels' combine, SetBlackWhitePoints, the chroma and hue steps, OpSave's colour branch
// (internal/fits/rgb.go, pixelops.go:441-550 and :679-692, tiff16.go:45-91, writejpg.go:43-89).  Kernels and host
// scalars in colour.hip.
#include "nlstack_frame_common.hpp"

extern "C" {

// the three planes named by planes[3]; the thread's error names `who`
static int rgb_planes(nl_stack_t *h, const int *planes, const char *who, nl::Planes *pl)
{
    if (!planes) return fail(NL_ERR_INVALID_ARG, "%s: null planes", who);
    for (int c = 0; c < 3; c++) {
        const int rc = resident_target(h, planes[c], who, false, &pl->p[c]);
        if (rc != NL_OK) return rc;
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
    float *s, *d;                                              // (-1, no other negative index: the last pass's result)
    rc = resident_target(src, src_idx, "frame_combine_from (source)", src_idx == -1, &s);
    if (rc == NL_OK) rc = resident_target(dst, dst_idx, "frame_combine_from (destination)", false, &d);
    if (rc != NL_OK) return rc;
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
    return need_whole_frame(h, who, "the blocks span rows");
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
    int rc = check_stars(who, stars, n_stars);
    if (rc == NL_OK) rc = need_whole_frame(h, who, "a star's disc spans rows");
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

static const int kHostPlanes[3] = {0, 1, 2};       // of a host form's own handle (host_frames_run with three planes)

int nl_rgb_balance(float *planar_host, int width, int height, const nl_star_t *stars, int n_stars, int block,
                   float border, float skip_bright, float skip_dim, nl_rgb_t shadows, nl_rgb_t highlights,
                   const float loc[3], const float scale[3], nl_rgb_balance_t *report, int device)
{
    if (!planar_host || width < 1 || height < 1) return fail(NL_ERR_INVALID_ARG, "rgb_balance: bad argument");
    if (const int rc = select_device(device); rc != NL_OK) return rc;
    return host_frames_run(3, planar_host, planar_host, width, height, device, [&](nl_stack_t *h) {
        nl::Planes pl;
        const int r = rgb_planes(h, kHostPlanes, "host planes", &pl);
        return r == NL_OK ? rgb_balance_impl(h, pl, "rgb_balance", stars, n_stars, block, border, skip_bright, skip_dim,
                                             shadows, highlights, loc, scale, report) : r;
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

int nl_stack_rgb_export(nl_stack_t *h, const int planes[3], float min, float max, float gamma, int bits, void *out_host)
{
    nl::Planes pl;
    NL_RGB_ENTRY(h, planes, "rgb_export", pl);
    const int rc = export_check("rgb_export", gamma, bits, out_host);
    return rc == NL_OK ? export_impl(h, nullptr, &pl, min, max, gamma, bits, out_host) : rc;
}

int nl_export_rgb(const float *planar_host, int64_t n, float min, float max, float gamma, int bits, void *out_host,
                  int device)
{
    if (!planar_host || n < 1 || n > 0x7fffffff) return fail(NL_ERR_INVALID_ARG, "export_rgb: bad argument");
    int rc = export_check("export_rgb", gamma, bits, out_host);
    if (rc == NL_OK) rc = select_device(device);
    if (rc != NL_OK) return rc;
    return host_frames_run(3, planar_host, nullptr, (int)n, 1, device, [&](nl_stack_t *h) {
        nl::Planes pl;
        const int r = rgb_planes(h, kHostPlanes, "host planes", &pl);
        return r == NL_OK ? export_impl(h, nullptr, &pl, min, max, gamma, bits, out_host) : r;
    });
}

}  // extern "C"
