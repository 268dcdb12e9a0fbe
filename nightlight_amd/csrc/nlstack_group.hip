// nlstack_group.hip -- nl_group_*: one stack fanned out over several GPUs from ONE process.
//
// The reference's Apply splits the pixel range over goroutines
// (internal/ops/stack/stack.go:142-152) and sums the two clip counters over them
// (:193-198).  A single-process host -- the Go CLI behind the cgo shim, the C++
// operator mirror -- gets the same split over the GPUs of the node here: tile t
// owns the rows tile_rows(height, n_tiles, t) of ALL frames on its own device, the
// passes of all tiles are enqueued before any is awaited, the result tiles land in
// disjoint row ranges of the caller's buffer, and the counters are summed on the
// host (two int64 per tile).  No pixel crosses devices, so there is no collective;
// the multi-process form of the same split (torch.distributed / RCCL) is
// nightlight_amd/dist.py.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <thread>
#include <vector>

#include "goal_seek.hpp"
#include "nlstack_internal.hpp"

struct nl_group {
    int n_frames = 0, width = 0, height = 0;
    std::vector<nl_stack_t *> tiles;
    std::vector<int> row0, rows;
    int distinct_devices = 1;
};

extern "C" {

void nl_group_tile_rows(int height, int n_tiles, int t, int *row0, int *rows)
{
    const int base = height / n_tiles, extra = height % n_tiles;
    if (rows) *rows = base + (t < extra ? 1 : 0);
    if (row0) *row0 = t * base + (t < extra ? t : extra);
}

void nl_group_destroy(nl_group_t *g)
{
    if (!g) return;
    for (nl_stack_t *h : g->tiles) nl_stack_destroy(h);
    delete g;
}

nl_group_t *nl_group_create(int n_frames, int width, int height, int n_tiles, const int *devices)
{
    int ndev = nl_device_count();
    if (ndev <= 0) return nullptr;                       // nl_last_error: no HIP device, no CPU path
    if (n_tiles <= 0) n_tiles = ndev;
    if (n_tiles > height) n_tiles = height > 0 ? height : 1;
    nl_group_t *g = new nl_group();
    g->n_frames = n_frames; g->width = width; g->height = height;
    for (int t = 0; t < n_tiles; t++) {
        int r0 = 0, nr = 0;
        nl_group_tile_rows(height, n_tiles, t, &r0, &nr);
        nl_stack_t *h = nl_stack_create(n_frames, width, height, r0, nr, devices ? devices[t] : t % ndev);
        if (!h) {
            nl_group_destroy(g);                          // destroy never touches the thread's error message
            return nullptr;
        }
        g->tiles.push_back(h);
        g->row0.push_back(r0);
        g->rows.push_back(nr);
    }
    {
        std::vector<int> seen;
        for (int t = 0; t < n_tiles; t++) {
            const int d = devices ? devices[t] : t % ndev;
            bool have = false;
            for (int s : seen) have = have || s == d;
            if (!have) seen.push_back(d);
        }
        g->distinct_devices = (int)seen.size();
    }
    return g;
}

int nl_group_size(nl_group_t *g) { return g ? (int)g->tiles.size() : 0; }

nl_stack_t *nl_group_tile(nl_group_t *g, int t)
{
    return (g && t >= 0 && t < (int)g->tiles.size()) ? g->tiles[(size_t)t] : nullptr;
}

}  // extern "C"

// Runs f(tile) for every tile, one host thread per tile beyond the first: staging a frame is a host memcpy
// into pinned memory per tile, and with one tile per device a serial loop would feed one DMA engine at a time.
// The first error (lowest tile) wins; its message becomes the calling thread's nl_last_error().
template <class F>
static int for_each_tile(nl_group_t *g, F &&f)
{
    const size_t n = g->tiles.size();
    std::vector<int> rc(n, NL_OK);
    std::vector<std::string> msg(n);
    auto one = [&](size_t t) {
        rc[t] = f(t);
        if (rc[t] != NL_OK) msg[t] = nl_last_error();        // (thread-local: fetch it on the worker)
    };
    std::vector<std::thread> workers;
    for (size_t t = 1; t < n; t++) workers.emplace_back(one, t);
    if (n > 0) one(0);
    for (auto &w : workers) w.join();
    for (size_t t = 0; t < n; t++)
        if (rc[t] != NL_OK) {
            nl::set_last_error(msg[t].c_str());
            return rc[t];
        }
    return NL_OK;
}

// Runs f(handle) tile after tile on the calling thread and stops at the first error, whose message stays the thread's: the
// setters, the stack of stacks, the finish of a goal-seek -- calls that wait on their device or are too short for a thread.
template <class F>
static int each_tile_in_turn(nl_group_t *g, F &&f)
{
    for (nl_stack_t *h : g->tiles) {
        const int rc = f(h);
        if (rc != NL_OK) return rc;
    }
    return NL_OK;
}

// The finish of a group pass on worker threads: when the tiles sit on more than one device (the copies of the result rows then
// run over separate links); NL_GROUP_PARALLEL_FINISH=1 / 0 forces it on / off (the tests force it on one device).
static bool finish_in_parallel(const nl_group_t *g)
{
    if (const char *e = getenv("NL_GROUP_PARALLEL_FINISH")) return e[0] == '1';
    return g->distinct_devices > 1;
}

extern "C" {

// every tile copies its rows out of the caller's frame into its own pinned staging buffer
// (pointer not retained, cgo rules) and starts its DMA; nothing is awaited on the devices
int nl_group_upload_frame(nl_group_t *g, int idx, const float *host_frame)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return for_each_tile(g, [&](size_t t) { return nl_stack_upload_frame_async(g->tiles[t], idx, host_frame); });
}

// F3 on the group: raw_host = the big-endian FITS payload of the WHOLE frame (width*height values); every tile
// takes the byte range of its rows (row-major: contiguous) through its pinned ring, decodes on its device
int nl_group_upload_frame_fits(nl_group_t *g, int idx, const void *raw_host, int bitpix, float bscale, float bzero,
                               float multiplier, float offset)
{
    if (!g || !raw_host) return NL_ERR_INVALID_ARG;
    const int bpv = bitpix < 0 ? -bitpix / 8 : bitpix / 8;
    return for_each_tile(g, [&](size_t t) {
        const char *part = static_cast<const char *>(raw_host) + (size_t)g->row0[t] * (size_t)g->width * (size_t)bpv;
        return nl_stack_upload_frame_fits_async(g->tiles[t], idx, part, bitpix, bscale, bzero, multiplier, offset);
    });
}

// F4 on the group: every tile receives the whole unaligned source frame and projects its own rows
int nl_group_upload_frame_projected(nl_group_t *g, int idx, const float *src_host, int src_w, int src_h,
                                    const float trans[6], float out_of_bounds, float multiplier, float offset)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return for_each_tile(g, [&](size_t t) {
        return nl_stack_upload_frame_projected_async(g->tiles[t], idx, src_host, src_w, src_h, trans, out_of_bounds,
                                                     multiplier, offset);
    });
}

// OpAlign's f.Project on the group: every tile projects its own rows from the resident source slot -- straight from
// it on the source's device, from a peer copy of the rows it needs on another one; nothing goes through host memory
int nl_group_frame_project_from(nl_group_t *g, int idx, nl_stack_t *src, int src_idx, const float trans[6],
                                float out_of_bounds)
{
    if (!g || !src) return NL_ERR_INVALID_ARG;
    const int rc = nl::stack_settle(src);                  // once, here: the tiles' threads only read the source
    if (rc != NL_OK) return rc;
    return for_each_tile(g, [&](size_t t) {
        return nl::stack_project_from(g->tiles[t], idx, src, src_idx, trans, out_of_bounds, "group_frame_project_from", true);
    });
}

// nl_group_frame_project_from with a bicubic or Lanczos-3 kernel (include/nlstack_resample.h, an extension)
int nl_group_frame_resample_from(nl_group_t *g, int idx, nl_stack_t *src, int src_idx, const float trans[6],
                                 float out_of_bounds, int kernel, int clamp)
{
    int rc = nl::resample_args_check("group_frame_resample_from", kernel, trans);     // in front of any device work
    if (rc != NL_OK) return rc;
    if (!g || !src) {
        nl::set_last_error(g ? "group_frame_resample_from: null handle" : "group_frame_resample_from: null group");
        return NL_ERR_INVALID_ARG;
    }
    if ((rc = nl::stack_settle(src)) != NL_OK) return rc;  // once, here: the tiles' threads only read the source
    return for_each_tile(g, [&](size_t t) {
        return nl::stack_project_from(g->tiles[t], idx, src, src_idx, trans, out_of_bounds, "group_frame_resample_from", true,
                                      kernel, clamp);
    });
}

int nl_group_fill_synthetic(nl_group_t *g, uint64_t seed)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_fill_synthetic(h, seed); });
}

int nl_group_set_active_frames(nl_group_t *g, int n)
{
    if (!g) return NL_ERR_INVALID_ARG;
    const int rc = each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_set_active_frames(h, n); });
    if (rc == NL_OK) g->n_frames = n;
    return rc;
}

int nl_group_set_weights(nl_group_t *g, const float *weights)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_set_weights(h, weights); });
}

int nl_group_set_exact(nl_group_t *g, int on)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_set_exact(h, on); });
}

}  // extern "C"

// One pass over the tiles, stack.go:142-210 over the devices: every tile's pass is started before any
// is awaited, every tile writes its own rows of the caller's buffers, the two counters are summed on the host.
static int run_tiles(nl_group_t *g, const nl::PassRequest &req, const nl::PassOutputs &to)
{
    // A failing tile must not leave the other tiles' passes enqueued and pending: every pass that was
    // started is also finished, and the FIRST error (with its message) is what the caller gets.
    int first_rc = NL_OK;
    std::string first_msg;
    auto note = [&](int rc) {
        if (rc != NL_OK && first_rc == NL_OK) { first_rc = rc; first_msg = nl_last_error(); }
    };
    const size_t n = g->tiles.size();
    size_t started = 0;
    for (; started < n && first_rc == NL_OK; started++)
        note(nl::stack_start(g->tiles[started], req));
    if (first_rc != NL_OK) started--;                     // (a failing start settles its handle: nothing of it is in flight)
    std::vector<int64_t> lo(n, 0), hi(n, 0);
    // tile t's finish: a wait and the copy of its rows; into the caller's buffers while all is well, nowhere after a failure
    auto finish = [&](size_t t) {
        const bool ok = first_rc == NL_OK;
        return nl::stack_finish(g->tiles[t], req, {ok ? to.out : nullptr, &lo[t], &hi[t], ok ? to.reject_low : nullptr,
                                                   ok ? to.reject_high : nullptr});
    };
    if (first_rc == NL_OK && finish_in_parallel(g)) {
        // one host thread per tile: the copies into the caller's (pageable) buffer -- 8 MiB of a 4096 x 4096 result per
        // tile of eight -- each run over their own device's link
        const int rc = for_each_tile(g, finish);
        if (rc != NL_OK) return rc;                       // (for_each_tile finished every tile and kept the first message)
    } else {
        for (size_t t = 0; t < started; t++) note(finish(t));
        if (first_rc != NL_OK) {
            nl::set_last_error(first_msg.c_str());
            return first_rc;
        }
    }
    int64_t sum_lo = 0, sum_hi = 0;                       // stack.go:193-198
    for (size_t t = 0; t < n; t++) { sum_lo += lo[t]; sum_hi += hi[t]; }
    if (to.clip_low) *to.clip_low = sum_lo;
    if (to.clip_high) *to.clip_high = sum_hi;
    return NL_OK;
}

static int null_group()
{
    nl::set_last_error("null group");
    return NL_ERR_INVALID_ARG;
}

using nl::MapsTier, nl::PassKind;

extern "C" {

// The pass entries: forwards to run_tiles.  (nl_group_run, like the setters, gives a null group its code without a message.)
int nl_group_run(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                 float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return run_tiles(g, {PassKind::Default, MapsTier::None, mode, sigma_low, sigma_high, ref_loc}, {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the weighted linear-fit pass (include/nlstack_wlinfit.h)
int nl_group_run_linfit_weighted(nl_group_t *g, float sigma_low, float sigma_high, float ref_loc,
                                 float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::WeightedLinfit, MapsTier::None, NL_ST_LINEAR_FIT, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the weighted clip pass whose weights follow their frames (include/nlstack_wclip.h); what can be told from the mode alone
// is told first, as nl_stack_run_clip_weighted_async does -- in the group's own words, and every tile checks again
int nl_group_run_clip_weighted(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    if (mode < NL_ST_MEDIAN || mode > NL_ST_AUTO) { nl::set_last_error("invalid stacking mode"); return NL_ERR_INVALID_MODE; }
    if (mode != NL_ST_AUTO && mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA) {
        nl::set_last_error("run_clip_weighted: the mode is neither NL_ST_SIGMA nor NL_ST_WINSOR_SIGMA");
        return NL_ERR_INVALID_MODE;
    }
    if (!g) return null_group();
    return run_tiles(g, {PassKind::WeightedClip, MapsTier::None, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the weighted MAD-sigma pass (include/nlstack_wmad.h)
int nl_group_run_mad_weighted(nl_group_t *g, float sigma_low, float sigma_high, float ref_loc,
                              float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::WeightedMad, MapsTier::None, NL_ST_MAD_SIGMA, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the deep pass (include/nlstack_deepstack.h)
int nl_group_run_deepstack(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::DeepStack, MapsTier::None, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the deep weighted MAD-sigma pass (include/nlstack_deepwmad.h)
int nl_group_run_mad_weighted_deepstack(nl_group_t *g, float sigma_low, float sigma_high, float ref_loc,
                                        float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::DeepWeightedMad, MapsTier::None, NL_ST_MAD_SIGMA, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the maps passes, one tier (nl::MapsTier) each
int nl_group_run_maps(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                      float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::Default, MapsTier::Column, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_group_run_maps_fast(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::Default, MapsTier::Fast, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_group_run_maps_resident(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::Default, MapsTier::Resident, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_group_run_maps_deep(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::Default, MapsTier::Deep, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_group_run_maps_full(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::Default, MapsTier::Full, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_group_run_maps_deepstack(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                                float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    if (!g) return null_group();
    return run_tiles(g, {PassKind::Default, MapsTier::DeepStack, mode, sigma_low, sigma_high, ref_loc},
                     {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

// every tile counts on its own device and writes its own rows
int nl_group_coverage(nl_group_t *g, uint16_t *coverage_host)
{
    if (!g) { nl::set_last_error("null group"); return NL_ERR_INVALID_ARG; }
    if (!coverage_host) { nl::set_last_error("coverage: null output"); return NL_ERR_INVALID_ARG; }
    return for_each_tile(g, [&](size_t t) { return nl_stack_coverage(g->tiles[t], coverage_host); });
}

int nl_group_last_mode(nl_group_t *g) { return (g && !g->tiles.empty()) ? nl_stack_last_mode(g->tiles[0]) : -1; }

// the goal-seek (goal_seek.hpp) with the counters summed over the tiles after every pass.  The mode is not checked here:
// an invalid one fails in the first pass, with the handle's code and message.
int nl_group_find_sigmas(nl_group_t *g, int mode, float ref_loc, float clip_perc_low, float clip_perc_high,
                         float *out_host, int64_t *clip_low, int64_t *clip_high,
                         float *sigma_low, float *sigma_high, int *passes)
{
    if (!g || g->tiles.empty()) return NL_ERR_INVALID_ARG;
    const int64_t total = (int64_t)g->width * g->height * (int64_t)g->n_frames;
    const int m = mode == NL_ST_AUTO ? nl::auto_select_mode(g->n_frames) : mode;
    return nl::goal_seek(
        m, clip_perc_low, clip_perc_high, total,
        [&](float lo, float hi, int64_t c[2]) { return nl_group_run(g, m, lo, hi, ref_loc, nullptr, &c[0], &c[1]); },
        [&](float lo, float hi) { return nl_group_run(g, m, lo, hi, ref_loc, nullptr, nullptr, nullptr); },
        [&] {
            if (!out_host) return NL_OK;
            return each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_finish(h, out_host, nullptr, nullptr); });
        },
        {clip_low, clip_high, sigma_low, sigma_high, passes});
}

// StackIncremental / StackIncrementalFinalize (stack.go:924-944) on every tile's device
int nl_group_accumulate(nl_group_t *g, float weight, int first)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_accumulate(h, weight, first); });
}

int nl_group_accumulate_finalize(nl_group_t *g, float weight_sum, float *out_host)
{
    if (!g) return NL_ERR_INVALID_ARG;
    return each_tile_in_turn(g, [&](nl_stack_t *h) { return nl_stack_accumulate_finalize(h, weight_sum, out_host); });
}

}  // extern "C"
