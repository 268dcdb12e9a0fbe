// nlstack_drizzle.hip -- the entries of include/nlstack_drizzle.h (AN EXTENSION: the reference has no drizzle): the
// geometry, laying a resident frame onto the two planes of a finer output grid, the quotient of the planes, and the
// rejection of a frame's outliers against a model; of include/nlstack_cfadrizzle.h (AN EXTENSION too): the same for
// one channel of a raw Bayer mosaic, the mosaic's transform and CosmeticCorrectionBayer in place on a resident mosaic;
// and of include/nlstack_sqdrizzle.h (AN EXTENSION too): the square kernel of both, the same checks under its names.
// One of the units of the frame steps (nlstack_frame_common.hpp); kernels in drizzle.hip, drizzle_cfa.hip,
// drizzle_square.hip and bayer.hip.
#include <math.h>

#include "bayer.hpp"
#include "drizzle.hpp"
#include "nlstack_frame_common.hpp"

namespace {

// The definition's geometry in double, rounded to fp32 once; what needs no handle of a drizzle call's arguments.  With
// sq the geometry of include/nlstack_sqdrizzle.h: the corners and the bounding box of the drop as well, and its R.
int drizzle_geometry(const char *who, const float *trans, float scale, float pixfrac, nl::DzGeom *out,
                     nl::DzSquare *sq = nullptr)
{
    if (!trans) return fail(NL_ERR_INVALID_ARG, "%s: null transform", who);
    if (!isfinite(scale) || !(scale > 0.0f)) return fail(NL_ERR_INVALID_ARG, "%s: scale %g (a finite number > 0)", who, scale);
    if (!(pixfrac > 0.0f && pixfrac <= 1.0f)) return fail(NL_ERR_INVALID_ARG, "%s: pixfrac %g (0 < pixfrac <= 1)", who, pixfrac);
    float unused[6];
    if (const int rc = invert_transform(trans, unused); rc != NL_OK) return rc;       // the reference's Invert test
    const double a = trans[0], b = trans[1], c = trans[2], d = trans[3], e = trans[4], f = trans[5];
    const double S = scale, p = pixfrac;
    const double Fa = S * a, Fb = S * b, Fc = S * (c + 0.5) - 0.5, Fd = S * d, Fe = S * e, Ff = S * (f + 0.5) - 0.5;
    const double det = Fa * Fe - Fb * Fd;
    const double Ga = Fe / det, Gb = -Fb / det, Gd = -Fd / det, Ge = Fa / det;
    const double Gc = -(Ga * Fc + Gb * Ff), Gf = -(Gd * Fc + Ge * Ff);
    const double hw = 0.5 * p * sqrt(fabs(det));
    const double reach = 0.5 + hw;
    double span = fmax((fabs(Ga) + fabs(Gb)) * reach, (fabs(Gd) + fabs(Ge)) * reach) + 0.5 + 1.0 / 64;
    nl::DzSquare corners = {{0, 0, 0, 0}, {0, 0, 0, 0}, 0, 0};
    if (sq) {
        const double h = 0.5 * p, ox[4] = {-h, -h, h, h}, oy[4] = {-h, h, h, -h};
        for (int k = 0; k < 4; k++) {
            const int from = det < 0 ? 3 - k : k;              // (either orientation: a positive edge sum)
            corners.cx[k] = (float)(Fa * ox[from] + Fb * oy[from]);
            corners.cy[k] = (float)(Fd * ox[from] + Fe * oy[from]);
        }
        const double bx = h * (fabs(Fa) + fabs(Fb)), by = h * (fabs(Fd) + fabs(Fe));
        const double reach_x = 0.5 + bx, reach_y = 0.5 + by;
        corners.bx = (float)bx;
        corners.by = (float)by;
        span = fmax(fabs(Ga) * reach_x + fabs(Gb) * reach_y, fabs(Gd) * reach_x + fabs(Ge) * reach_y) + 0.5 + 1.0 / 64;
    }
    const nl::DzGeom g = {{(float)Fa, (float)Fb, (float)Fc, (float)Fd, (float)Fe, (float)Ff},
                          {(float)Ga, (float)Gb, (float)Gc, (float)Gd, (float)Ge, (float)Gf}, (float)hw, 0};
    const float all[23] = {g.f.a, g.f.b, g.f.c, g.f.d, g.f.e, g.f.f, g.g.a, g.g.b, g.g.c, g.g.d, g.g.e, g.g.f, g.hw,
                           corners.cx[0], corners.cx[1], corners.cx[2], corners.cx[3], corners.cy[0], corners.cy[1],
                           corners.cy[2], corners.cy[3], corners.bx, corners.by};
    for (float v : all)
        if (!isfinite(v)) return fail(NL_ERR_INVALID_ARG, "%s: a coefficient of the geometry is not finite", who);
    const double R = ceil(span);
    if (!(R <= (double)NL_DZ_MAX_RADIUS))
        return fail(NL_ERR_INVALID_ARG, "%s: window radius %.0f beyond NL_DZ_MAX_RADIUS %d (the output grid is too coarse for this frame)",
                    who, R, NL_DZ_MAX_RADIUS);
    *out = g;
    out->radius = (int)R;
    if (sq) *sq = corners;
    return NL_OK;
}

// what the channel and the CFA of a CFA entry name: a NULL or empty name, then the reference's two messages, CFA first;
// *id = bayer.hpp's BayerChannel
int channel_of(const char *who, const char *channel, const char *cfa, nl::DzChannel *out, int *id = nullptr)
{
    if (!channel || !cfa || !*channel || !*cfa) return fail(NL_ERR_INVALID_ARG, "%s needs a channel and a CFA", who);
    int ch, xo, yo;
    if (const int rc = cfa_names(channel, cfa, &ch, &xo, &yo); rc != NL_OK) return rc;
    *out = nl::dz_channel(ch, xo, yo);
    if (id) *id = ch;
    return NL_OK;
}

// an entry's name as its messages say it: alone, and for its three slots
struct DzWho { const char *who, *source, *sum, *wgt; };
#define NL_DZ_WHO(name) {name, name " (source)", name " (sum plane)", name " (weight plane)"}

// developer switches of the square drizzle as launch_drizzle_square takes them
unsigned square_switches(const nl_stack *h)
{
    return project_switches(h) | ((h->dev_flags & kDevSquareEveryCandidate) ? nl::kDzSquareEveryCandidate : 0u);
}

// nl_stack_frame_drizzle_from and, with cfa_form, nl_stack_frame_drizzle_cfa_from: the same checks in the same order
// under the entry's own name, the names of the CFA form behind the kernel and the weight; with square the two
// square entries, which have no kernel to check
int drizzle_from(const DzWho &names, nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                 const float *trans, float scale, float pixfrac, float weight, int first, int kernel, bool cfa_form,
                 const char *channel, const char *cfa, bool square = false)
{
    const char *who = names.who;
    // in front of any device work: what needs no handle
    if (!trans) return fail(NL_ERR_INVALID_ARG, "%s: null transform", who);
    if (!square && kernel != NL_DZ_TURBO && kernel != NL_DZ_POINT)
        return fail(NL_ERR_INVALID_ARG, "%s: unknown kernel %d (NL_DZ_TURBO 0, NL_DZ_POINT 1)", who, kernel);
    if (!isfinite(weight) || !(weight > 0.0f)) return fail(NL_ERR_INVALID_ARG, "%s: weight %g (a finite number > 0)", who, weight);
    nl::DzChannel ch = {0, 0, 0, 0, 0};
    int rc = cfa_form ? channel_of(who, channel, cfa, &ch) : NL_OK;
    if (rc != NL_OK) return rc;
    nl::DzGeom geom;
    nl::DzSquare sq;
    rc = drizzle_geometry(who, trans, scale, pixfrac, &geom, square ? &sq : nullptr);
    if (rc != NL_OK) return rc;
    if (!dst || !src) return fail(NL_ERR_INVALID_ARG, "%s: null handle", who);
    NL_CHECK_HANDLE(src);
    NL_CHECK_HANDLE(dst);
    if (src->device != dst->device)
        return fail(NL_ERR_INVALID_ARG, "%s: source on device %d, destination on device %d", who, src->device, dst->device);
    if (sum_idx == wgt_idx) return fail(NL_ERR_INVALID_ARG, "%s: slot %d is both the sum and the weight plane", who, sum_idx);
    float *s = nullptr, *d_sum = nullptr, *d_wgt = nullptr;
    rc = resident_target(src, src_idx, names.source, false, &s);
    if (rc == NL_OK) rc = resident_target(dst, sum_idx, names.sum, false, &d_sum);
    if (rc == NL_OK) rc = resident_target(dst, wgt_idx, names.wgt, false, &d_wgt);
    if (rc == NL_OK) rc = need_whole_image(src, names.source, "a drizzle reads any row of the source");
    if (rc == NL_OK) rc = need_int32_pixels(src->npix, who, "source frame");
    if (rc == NL_OK) rc = need_int32_pixels(dst->npix, who, "destination tile");
    if (rc != NL_OK) return rc;
    if (dst->d_frames != dst->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "%s: the destination's frames are attached, not owned", who);
    if (s == d_sum || s == d_wgt)
        return fail(NL_ERR_INVALID_ARG, "%s: slot %d of one handle is source and destination (a drizzle cannot run in place)", who, src_idx);
    if (src != dst && (rc = nl_stack_order_stream_after(src, dst->stream)) != NL_OK) return rc;
    NL_HIP(hipSetDevice(dst->device));
    if (square && cfa_form)
        NL_HIP(nl::launch_drizzle_square_cfa(s, src->width, src->height, d_sum, d_wgt, dst->width, dst->row0, dst->rows, geom,
                                             sq, weight, first != 0, ch, square_switches(dst), dst->stream));
    else if (square)
        NL_HIP(nl::launch_drizzle_square(s, src->width, src->height, d_sum, d_wgt, dst->width, dst->row0, dst->rows, geom, sq,
                                         weight, first != 0, square_switches(dst), dst->stream));
    else if (cfa_form)
        NL_HIP(nl::launch_drizzle_cfa(s, src->width, src->height, d_sum, d_wgt, dst->width, dst->row0, dst->rows, geom, weight,
                                      first != 0, kernel == NL_DZ_POINT, ch, project_switches(dst), dst->stream));
    else
        NL_HIP(nl::launch_drizzle(s, src->width, src->height, d_sum, d_wgt, dst->width, dst->row0, dst->rows, geom, weight,
                                  first != 0, kernel == NL_DZ_POINT, project_switches(dst), dst->stream));
    NL_HIP(hipStreamSynchronize(dst->stream));                 // the caller may overwrite the source slot at once
    return NL_OK;
}

// nl_stack_drizzle_tile_paths and, with square, nl_stack_drizzle_square_tile_paths (the window of the square R)
int tile_paths(const char *who, nl_stack_t *dst, nl_stack_t *src, int src_idx, const float *trans, float scale, float pixfrac,
               int64_t *staged, int64_t *direct, bool square)
{
    if (!dst || !src || !trans || !staged || !direct) return fail(NL_ERR_INVALID_ARG, "%s: null argument", who);
    nl::DzGeom geom;
    nl::DzSquare sq;
    const int rc = drizzle_geometry(who, trans, scale, pixfrac, &geom, square ? &sq : nullptr);
    if (rc != NL_OK) return rc;
    if (src_idx < 0 || src_idx >= src->n_frames)               // (a host query: no device, no stream is touched)
        return fail(NL_ERR_INVALID_ARG, "%s: bad index %d", who, src_idx);
    const float *s = src->d_frames + (int64_t)src_idx * src->fstride;
    nl::drizzle_tile_paths(s, src->width, src->height, dst->width, dst->row0, dst->rows, geom, project_switches(dst),
                           staged, direct);
    return NL_OK;
}

// what nl_stack_frame_reject_against and its CFA form return: the workgroups' counts, added
int reject_counts(nl_stack_t *h, unsigned long long *counts, int64_t *n_low, int64_t *n_high)
{
    std::vector<unsigned long long> part(2 * (size_t)kStatBlocks);
    NL_HIP(hipMemcpyAsync(part.data(), counts, sizeof(unsigned long long) * part.size(), hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    int64_t lo = 0, hi = 0;
    for (int b = 0; b < kStatBlocks; b++) {
        lo += (int64_t)part[2 * (size_t)b];
        hi += (int64_t)part[2 * (size_t)b + 1];
    }
    if (n_low) *n_low = lo;
    if (n_high) *n_high = hi;
    return NL_OK;
}

}  // namespace

extern "C" {

int nl_drizzle_geometry(const float trans[6], float scale, float pixfrac, float src_to_out[6], float out_to_src[6],
                        float *half_width, int *radius)
{
    if (!trans || !src_to_out || !out_to_src || !half_width || !radius)
        return fail(NL_ERR_INVALID_ARG, "drizzle_geometry: null argument");
    nl::DzGeom g;
    const int rc = drizzle_geometry("drizzle_geometry", trans, scale, pixfrac, &g);
    if (rc != NL_OK) return rc;
    const float F[6] = {g.f.a, g.f.b, g.f.c, g.f.d, g.f.e, g.f.f}, G[6] = {g.g.a, g.g.b, g.g.c, g.g.d, g.g.e, g.g.f};
    memcpy(src_to_out, F, sizeof F);
    memcpy(out_to_src, G, sizeof G);
    *half_width = g.hw;
    *radius = g.radius;
    return NL_OK;
}

int nl_stack_frame_drizzle_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                const float trans[6], float scale, float pixfrac, float weight, int first, int kernel)
{
    return drizzle_from(NL_DZ_WHO("frame_drizzle_from"), dst, sum_idx, wgt_idx, src, src_idx, trans, scale, pixfrac, weight, first,
                        kernel, false, nullptr, nullptr);
}

int nl_stack_frame_drizzle_cfa_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                    const float trans[6], float scale, float pixfrac, float weight, int first,
                                    int kernel, const char *channel, const char *cfa)
{
    return drizzle_from(NL_DZ_WHO("frame_drizzle_cfa_from"), dst, sum_idx, wgt_idx, src, src_idx, trans, scale, pixfrac, weight,
                        first, kernel, true, channel, cfa);
}

int nl_stack_drizzle_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], float scale,
                                float pixfrac, int64_t *staged, int64_t *direct)
{
    return tile_paths("drizzle_tile_paths", dst, src, src_idx, trans, scale, pixfrac, staged, direct, false);
}

int nl_stack_drizzle_finalize(nl_stack_t *h, int sum_idx, int wgt_idx, int out_idx, float min_weight, float empty)
{
    float *d_sum = nullptr, *d_wgt = nullptr, *d_out = nullptr;
    int rc = resident_entry(h, sum_idx, "drizzle_finalize (sum plane)", false, &d_sum);
    if (rc == NL_OK) rc = resident_target(h, wgt_idx, "drizzle_finalize (weight plane)", false, &d_wgt);
    if (rc == NL_OK) rc = resident_target(h, out_idx, "drizzle_finalize (result)", false, &d_out);
    if (rc != NL_OK) return rc;
    NL_HIP(nl::launch_drizzle_finalize(d_sum, d_wgt, d_out, h->npix, min_weight, empty, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl_stack_frame_reject_against(nl_stack_t *h, int idx, int model_idx, float low, float high, int64_t *n_low,
                                  int64_t *n_high)
{
    if (!(low >= 0.0f) || !(high >= 0.0f))                     // (in front of the handle; a NaN fails the comparison)
        return fail(NL_ERR_INVALID_ARG, "frame_reject_against: low %g, high %g (absolute thresholds >= 0)", low, high);
    float *d = nullptr, *m = nullptr;
    int rc = resident_entry(h, idx, "frame_reject_against", false, &d);
    if (rc == NL_OK) rc = resident_target(h, model_idx, "frame_reject_against (model)", false, &m);
    if (rc != NL_OK) return rc;
    // two words per workgroup in the statistics' partials (kStatBlocks x 3 doubles)
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(h->d_stat_partial);
    NL_HIP(nl::launch_reject_against(d, m, h->npix, low, high, counts, kStatBlocks, h->stream));
    return reject_counts(h, counts, n_low, n_high);
}

int nl_stack_frame_reject_against_cfa(nl_stack_t *h, int idx, int model_idx, const char *channel, const char *cfa,
                                      float low, float high, int64_t *n_low, int64_t *n_high)
{
    if (!(low >= 0.0f) || !(high >= 0.0f))                     // (in front of the handle; a NaN fails the comparison)
        return fail(NL_ERR_INVALID_ARG, "frame_reject_against_cfa: low %g, high %g (absolute thresholds >= 0)", low, high);
    nl::DzChannel ch;
    int rc = channel_of("frame_reject_against_cfa", channel, cfa, &ch);
    if (rc != NL_OK) return rc;
    float *d = nullptr, *m = nullptr;
    rc = resident_entry(h, idx, "frame_reject_against_cfa", false, &d);
    if (rc == NL_OK) rc = resident_target(h, model_idx, "frame_reject_against_cfa (model)", false, &m);
    if (rc != NL_OK) return rc;
    unsigned long long *counts = reinterpret_cast<unsigned long long *>(h->d_stat_partial);
    NL_HIP(nl::launch_reject_against_cfa(d, m, h->width, h->row0, h->rows, ch, low, high, counts, kStatBlocks, h->stream));
    return reject_counts(h, counts, n_low, n_high);
}

int nl_drizzle_square_geometry(const float trans[6], float scale, float pixfrac, float src_to_out[6], float out_to_src[6],
                               float corners[8], float box_half[2], int *radius)
{
    if (!trans || !src_to_out || !out_to_src || !corners || !box_half || !radius)
        return fail(NL_ERR_INVALID_ARG, "drizzle_square_geometry: null argument");
    nl::DzGeom g;
    nl::DzSquare sq;
    const int rc = drizzle_geometry("drizzle_square_geometry", trans, scale, pixfrac, &g, &sq);
    if (rc != NL_OK) return rc;
    const float F[6] = {g.f.a, g.f.b, g.f.c, g.f.d, g.f.e, g.f.f}, G[6] = {g.g.a, g.g.b, g.g.c, g.g.d, g.g.e, g.g.f};
    memcpy(src_to_out, F, sizeof F);
    memcpy(out_to_src, G, sizeof G);
    for (int k = 0; k < 4; k++) {
        corners[2 * k] = sq.cx[k];
        corners[2 * k + 1] = sq.cy[k];
    }
    box_half[0] = sq.bx;
    box_half[1] = sq.by;
    *radius = g.radius;
    return NL_OK;
}

int nl_stack_frame_drizzle_square_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                       const float trans[6], float scale, float pixfrac, float weight, int first)
{
    return drizzle_from(NL_DZ_WHO("frame_drizzle_square_from"), dst, sum_idx, wgt_idx, src, src_idx, trans, scale, pixfrac,
                        weight, first, 0, false, nullptr, nullptr, true);
}

int nl_stack_frame_drizzle_square_cfa_from(nl_stack_t *dst, int sum_idx, int wgt_idx, nl_stack_t *src, int src_idx,
                                           const float trans[6], float scale, float pixfrac, float weight, int first,
                                           const char *channel, const char *cfa)
{
    return drizzle_from(NL_DZ_WHO("frame_drizzle_square_cfa_from"), dst, sum_idx, wgt_idx, src, src_idx, trans, scale, pixfrac,
                        weight, first, 0, true, channel, cfa, true);
}

int nl_stack_drizzle_square_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6], float scale,
                                       float pixfrac, int64_t *staged, int64_t *direct)
{
    return tile_paths("drizzle_square_tile_paths", dst, src, src_idx, trans, scale, pixfrac, staged, direct, true);
}

int nl_drizzle_cfa_transform(const float trans_debayered[6], const char *cfa, float trans_raw[6])
{
    if (!trans_debayered || !trans_raw || !cfa || !*cfa) return fail(NL_ERR_INVALID_ARG, "drizzle_cfa_transform: null argument");
    int xo, yo;
    if (const int rc = cfa_offsets(cfa, &xo, &yo); rc != NL_OK) return rc;
    const double a = trans_debayered[0], b = trans_debayered[1], c = trans_debayered[2];
    const double d = trans_debayered[3], e = trans_debayered[4], f = trans_debayered[5];
    // plane pixel (x, y) is mosaic pixel (x + xo, y + yo) (debayer.go:87-90): T(i - xo, j - yo)
    const float out[6] = {(float)a, (float)b, (float)(c - a * xo - b * yo), (float)d, (float)e, (float)(f - d * xo - e * yo)};
    for (int k = 0; k < 6; k++)
        if (!isfinite(trans_debayered[k]) || !isfinite(out[k]))
            return fail(NL_ERR_INVALID_ARG, "drizzle_cfa_transform: a coefficient is not finite");
    memcpy(trans_raw, out, sizeof out);
    return NL_OK;
}

int nl_stack_frame_badpixel_cfa(nl_stack_t *h, int idx, const char *channel, const char *cfa, float sigma_low,
                                float sigma_high, int64_t *removed_out, float *stats_out)
{
    int rc = nl::require_device();            // (as nl_stack_upload_frame_cfa: without a device NL_ERR_NO_DEVICE)
    if (rc != NL_OK) return rc;
    float *d = nullptr;
    if ((rc = resident_entry(h, idx, "frame_badpixel_cfa", false, &d)) != NL_OK) return rc;
    nl::DzChannel ch;
    int chan;
    if ((rc = channel_of("frame_badpixel_cfa", channel, cfa, &ch, &chan)) != NL_OK) return rc;
    if ((rc = need_whole_frame(h, "frame_badpixel_cfa", "3x3 stencil, whole-frame std")) != NL_OK) return rc;
    nl::BayerParams p;
    p.mean = p.std = NAN;
    p.removed = 0;
    if (sigma_low != 0.0f && sigma_high != 0.0f) {             // preprocess.go:181-183
        const nl::BayerGeom g = nl::bayer_geom(h->width, h->height, chan, ch.xo, ch.yo);
        nl::BayerScratch s;
        auto carve = [&](void *base) {                         // (the compact buffers only: the mosaic stays in its slot)
            nl::Carver cv(base);
            s.delta = cv.take<float>((size_t)g.rows * g.cstride);
            s.median = cv.take<float>((size_t)g.rows * g.cstride);
            s.rowsum = cv.take<float>((size_t)g.rows);
            s.removed = cv.take<unsigned>((size_t)nl::bayer_replace_blocks(g));
            s.params = cv.take<nl::BayerParams>(1);
            return cv.bytes();
        };
        NL_HIP(h->frame_scratch.cfa.reserve(carve(nullptr), h->stream));
        carve(h->frame_scratch.cfa.ptr);
        NL_HIP(nl::launch_bayer_correct(d, g, sigma_low, sigma_high, s, h->stream));
        NL_HIP(hipMemcpyAsync(&p, s.params, sizeof p, hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    if (removed_out) *removed_out = (int64_t)p.removed;
    if (stats_out) { stats_out[0] = p.mean; stats_out[1] = p.std; }
    return NL_OK;
}

}  // extern "C"
