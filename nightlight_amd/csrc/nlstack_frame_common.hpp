// nlstack_frame_common.hpp -- what the units of the frame steps (nlstack_frame.hip, nlstack_frame_pre.hip,
// nlstack_frame_stretch.hip, nlstack_frame_rgb.hip, nlstack_drizzle.hip) ask of a handle before they launch, and the plumbing around their
// launches, each written once.  Defined in nlstack_frame.hip unless a template.  Private like nlstack_internal.hpp.
#pragma once

#include "nlstack_internal.hpp"

namespace nl {

// The pixels a call means, *d (h is checked): slot idx of h once its pending uploads have landed, "<who>: bad index
// <idx>" outside [0, n_frames); idx < 0 with result_ok the last pass's result, "<who>: the handle has not run a pass"
// without one.  resident_entry: NL_CHECK_HANDLE ("null handle", the handle's device) first.
int resident_target(nl_stack_t *h, int idx, const char *who, bool result_ok, float **d);
int resident_entry(nl_stack_t *h, int idx, const char *who, bool result_ok, float **d);
// a step that looks beyond its own pixel (why) cannot run on a tile of rows; its kernels index pixels with 32 bits;
// need_whole_frame: both, of h's own frame
int need_whole_image(const nl_stack_t *h, const char *who, const char *why);
int need_int32_pixels(int64_t n, const char *who, const char *what = "frame");
int need_whole_frame(const nl_stack_t *h, const char *who, const char *why);
// an output array of `capacity` elements at ptr; a list of n_stars stars; the arguments of the gray and colour export
int check_capacity(const char *who, int capacity, const void *ptr);
int check_stars(const char *who, const nl_star_t *stars, int n_stars);
int export_check(const char *who, float gamma, int bits, const void *out_host);
// The names of the colour-camera entries (neither null): the CFA, then the channel, as the reference checks them --
// "Unknown CFA value <cfa>", "Unknown debayering value <channel>".  (*xo, *yo) = getOffsets (debayer.go:26-37); *ch =
// bayer.hpp's BayerChannel (kBayerR / kBayerG / kBayerB)
int cfa_offsets(const char *cfa, int *xo, int *yo);
int cfa_names(const char *channel, const char *cfa, int *ch, int *xo, int *yo);

// What a reduction enqueued on h->stream leaves in h->d_stat_partial; each waits for the stream.  The kStatBlocks
// per-block fp64 sums added from block 0 on (the order is part of the result's bits):
int sum_stat_partials(nl_stack_t *h, double *sum);
// the per-block {min, sum, max} partials of launch_min_sum_max folded from block 0 on: compared in fp32, summed in
// fp64 in block order (bit-exact against the reference); min / mean / max of n values from such partials
// (launch_min_sum_max, or a tone curve or clamp that reduces what it writes) in h->d_stat_partial, or in d_part
struct MinSumMax { float lo; double sum; float hi; };
MinSumMax fold_min_sum_max(const std::vector<double> &part);
int min_mean_max_from_partials(nl_stack_t *h, int64_t n, float *mn, float *mean, float *mx, const double *d_part = nullptr);
// nl_stack_frame_stats on the n floats at d
int frame_stats_impl(nl_stack_t *h, const float *d, int64_t n, float *mn, float *mean, float *mx, double *variance);

// The host forms: n_planes frames of host memory, one behind the other at in_host, on a width x height handle of the
// call's own (with_scratch_frames): up into slots 0 .. n_planes - 1, run(h), and with out_host back down the same way
template <class Run>
int host_frames_run(int n_planes, const float *in_host, float *out_host, int width, int height, int device, Run run)
{
    return with_scratch_frames(n_planes, width, height, device, [&](nl_stack_t *h) {
        const size_t n = (size_t)width * (size_t)height;
        int r = NL_OK;
        for (int c = 0; c < n_planes && r == NL_OK; c++) r = nl_stack_upload_tile(h, c, in_host + n * c);
        if (r == NL_OK) r = run(h);
        for (int c = 0; c < n_planes && r == NL_OK && out_host; c++) r = nl_stack_download_tile(h, c, out_host + n * c);
        return r;
    });
}

// OpSave's quantisation of the npix floats at `gray`, or of the planes `rgb` as R G B A: the counts through the handle's
// ingest buffer (like nl_stack_download_result_fits) down into out_host
int export_impl(nl_stack_t *h, const float *gray, const Planes *rgb, float min, float max, float gamma, int bits,
                void *out_host);

}  // namespace nl

using nl::cfa_names, nl::cfa_offsets, nl::check_capacity, nl::check_stars, nl::export_check, nl::export_impl, nl::frame_stats_impl, nl::host_frames_run,
    nl::min_mean_max_from_partials, nl::need_int32_pixels, nl::need_whole_frame, nl::need_whole_image, nl::resident_entry, nl::resident_target,
    nl::sum_stat_partials;
