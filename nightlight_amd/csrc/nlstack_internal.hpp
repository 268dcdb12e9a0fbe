// nlstack_internal.hpp -- what the units of the C ABI (nlstack_api.hip, nlstack_pass.hip, nlstack_group.hip and, through
// nlstack_frame_common.hpp, nlstack_frame.hip, nlstack_frame_pre.hip, nlstack_frame_stretch.hip, nlstack_frame_rgb.hip)
// share: the handle and the error state (the allocator and the scratch types: dev_memory.hpp).  Private: no kernel
// source includes it, not installed.
#pragma once

#include <string.h>

#include <string>
#include <vector>

#include "background.hpp"
#include "blur.hpp"
#include "colour.hpp"
#include "deband.hpp"
#include "dev_memory.hpp"
#include "locscale.hpp"
#include "project.hpp"
#include "stars.hpp"
#include "tone.hpp"
#include "stack_kernels.h"

namespace nl {

extern thread_local std::string g_err;     // what nl_last_error() returns on this thread
int fail(int code, const char *fmt, ...);   // g_err = the formatted message; returns code

// NL_ERR_NO_DEVICE unless HIP sees a device (*count: how many); select_device: that, a range check, hipSetDevice
int require_device(int *count = nullptr);
int select_device(int device);

// The host forms of the frame steps (nl_fits_decode, nl_find_stars, ...): a one-frame width x height handle of their
// own per call carries stream and scratch, so concurrent calls share nothing.  run(h) runs on it; its error message
// outlives the handle.  A handle that cannot be created gives NL_ERR_HIP with nl_stack_create's message.
template <class Run>
int with_scratch_frames(int n_frames, int width, int height, int device, Run run)
{
    nl_stack_t *h = nl_stack_create(n_frames, width, height, 0, height, device);
    if (!h) return NL_ERR_HIP;
    const int rc = run(h);
    const std::string keep = g_err;
    nl_stack_destroy(h);
    g_err = keep;
    return rc;
}
template <class Run>
int with_scratch_handle(int width, int height, int device, Run run)
{
    return with_scratch_frames(1, width, height, device, run);
}

// the inverse of the forward Transform2D t (internal/star/coord.go:159-199, fp32 as written there); a singular one is
// NL_ERR_INVALID_ARG "Matrix has no inverse" (nlstack_api.hip)
int invert_transform(const float t[6], float inv[6]);

// Which engines a maps pass may run on.  Ordered: every tier includes the ones below it.
enum class MapsTier {
    None,                 // no maps pass
    Column,               // nl_stack_run_maps (include/nlstack_maps.h): the column kernel, every mode
    Fast,                 // nl_stack_run_maps_fast (include/nlstack_fastmaps.h): and the register-resident sigma / winsorized kernels, 2 ... 128 frames
    Resident,             // nl_stack_run_maps_resident (include/nlstack_residentmaps.h): and the linear fit's kernels and cascade
    Deep,                 // nl_stack_run_maps_deep (include/nlstack_deepmaps.h): and the LDS-column sigma / winsorized kernels, 129 ... 512 frames
    Full,                 // nl_stack_run_maps_full (include/nlstack_fullmaps.h): and the MAD-sigma kernels, 1 ... 512 frames; the median on its default kernels
    DeepStack,            // nl_stack_run_maps_deepstack (include/nlstack_deepstackmaps.h): and MAD sigma / the median of 513 ... 2048 frames on
                          // 8 / 16 lanes per pixel; sigma / winsorized clipping beyond 512 frames on the wave-per-pixel replay
};
// the kinds of pass: select_engine (nlstack_pass.hip) gives every kind but Default an engine of its own
enum class PassKind {
    Default,              // nl_stack_run_async and, with a tier, the nl_stack_run_maps* entries
    WeightedLinfit,       // nl_stack_run_linfit_weighted (include/nlstack_wlinfit.h): run_linfit_weighted; mode is NL_ST_LINEAR_FIT
    WeightedClip,         // nl_stack_run_clip_weighted (include/nlstack_wclip.h): run_clip_weighted
    WeightedMad,          // nl_stack_run_mad_weighted (include/nlstack_wmad.h): run_mad_weighted; mode is NL_ST_MAD_SIGMA
    DeepStack,            // nl_stack_run_deepstack (include/nlstack_deepstack.h): the median / MAD sigma of 513 ... 2048 frames on
                          // 8 / 16 lanes per pixel (run_deep_median, run_deep_mad); everything else is the Default pass
    DeepWeightedMad,      // nl_stack_run_mad_weighted_deepstack (include/nlstack_deepwmad.h): WeightedMad of 513 ... 2048 frames on
                          // run_deep_mad_weighted; everything else is the WeightedMad pass
};
// One stack pass as every pass entry of the handle and of the group asks for it, and where its results go; any output
// may be null, the two maps are read by a maps pass only.
struct PassRequest {
    PassKind kind;
    MapsTier tier;
    int mode;
    float sigma_low, sigma_high, ref_loc;
};
struct PassOutputs {
    float *out;
    int64_t *clip_low, *clip_high;
    uint16_t *reject_low, *reject_high;
};
// The two halves of a pass (nlstack_pass.hip), so that the group (nlstack_group.hip) starts every tile before it awaits
// any.  stack_start enqueues; a failing one leaves nothing in flight on the handle.  stack_finish waits and copies out:
// nl_stack_finish, with the two planes of the map behind a maps request.
int stack_start(nl_stack_t *h, const PassRequest &req);
int stack_finish(nl_stack_t *h, const PassRequest &req, const PassOutputs &to);
int auto_select_mode(int n_frames);         // stack.go:45-55: what NL_ST_AUTO stands for

}  // namespace nl

using nl::cached_free, nl::cached_malloc, nl::dev_malloc, nl::fail, nl::g_err, nl::invert_transform, nl::select_device, nl::with_scratch_frames, nl::with_scratch_handle;

#define NL_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(NL_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                                \
    } while (0)

constexpr int kTimingRing = 64;     // passes whose HIP-event times can be read back after the fact
constexpr int kStageSlots = 4;      // pinned staging buffers of the asynchronous upload
constexpr int kStatBlocks = 2048;
constexpr int kOrderRing = 8;              // events nl_stack_order_stream_after cycles through
// per-pass device scratch, zeroed by one memset (or, in the fused protocol of the sigma / winsorized fast path, by
// the previous pass's dominant kernel -- two sets alternate): clip accumulators + list lengths + snapshot
constexpr size_t kScratchBytes = sizeof(unsigned long long) * nl::kScratchWords;

// what a pass leaves behind: filled in by its engine, kept on the handle as `last`
struct PassFacts {
    bool has_counters = false;    // d_counters holds the pass's clip counters
    bool used_fast = false;       // a dominant kernel handed pixels over: the list lengths belong to this pass
    bool lists = false;           // ... and sit behind the totals (d_counters[2])
    bool fused = false;           // fused protocol: this pass's scratch set used, the other one zeroed
    bool tail_fused = false;      // generic pass + first replay ran as one launch (stack_tail_fused.hip)
    bool zeroed_behind = false;   // the reduction kernel left the scratch set zeroed
};

struct nl_stack {
    int device = 0;
    int n_frames = 0, width = 0, height = 0, row0 = 0, rows = 0;
    int n_capacity = 0;               // frame slots allocated; n_frames <= n_capacity are in use (nl_stack_set_active_frames)
    int64_t npix = 0;                 // rows*width
    int64_t fstride = 0;              // floats between consecutive frames of the buffer d_frames points at
    int64_t fstride_owned = 0;        // ... of the owned buffer (padded_frame_stride); a lent buffer brings its own
    hipStream_t stream = nullptr;
    // HIP events of the last kTimingRing passes (whole pass; dominant kernel only), so a caller can
    // queue many passes without a host sync and read every pass's GPU time afterwards
    hipEvent_t ring_start[kTimingRing] = {}, ring_stop[kTimingRing] = {};
    hipEvent_t ring_dom0[kTimingRing] = {}, ring_dom1[kTimingRing] = {};
    bool ring_dom0_is_start[kTimingRing] = {};            // the pass recorded one event for both (nothing ran in between)
    bool ring_timed[kTimingRing] = {};                    // the pass in this slot recorded its timing events (not with developer switch 32)
    int64_t pass_seq = 0;                                  // passes enqueued so far
    int64_t copy_waits_pass = 0;                           // pass the copy stream has been ordered behind
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;      // = the ring slot of the current / last pass
    hipEvent_t ev_dom0 = nullptr, ev_dom1 = nullptr;
    hipStream_t side_stream = nullptr;                     // replay of the dominant kernel's hand-overs,
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;        // concurrent with the generic pass
    hipEvent_t ev_order[kOrderRing] = {};                   // nl_stack_order_stream_after
    int order_seq = 0;
    unsigned ev_rel = 0;                                   // creation flag of the pass's events (hipEventDisableSystemFence or 0)
    float *d_frames_owned = nullptr;  // [n_capacity][fstride_owned], the first npix floats of a slot in use
    float *d_frames = nullptr;        // owned or lent
    float *d_out = nullptr;           // [npix]
    float *d_acc = nullptr;           // stack-of-stacks accumulator, lazily allocated
    float *d_weights = nullptr;       // [n_frames]
    bool has_weights = false;
    float *d_xstat = nullptr;         // [(n_frames+1)*2]
    unsigned long long *d_sets = nullptr;      // two scratch sets of kScratchWords; d_partial = the current one
    int cur_set = 0;
    bool sets_clean = false;                   // both sets as a fused pass leaves them: the current one used, the other zeroed
    bool partial_clean = false;                // the current set is all zeros: the last pass's reduction kernel left it so (plain protocol of the sigma fast path)
    unsigned long long *d_partial = nullptr;   // [kClipSlots][2] clip accumulators + 2 words of list lengths
    float2 *d_bounds = nullptr;                // decision pass of weighted stacks: [kBoundRounds][npix] thresholds, lazily allocated
    unsigned char *d_nrounds = nullptr;        // [npix]
    bool bounds_tried = false;
    // maps (nl_stack_run_maps / nl_stack_coverage), allocated by the first call that needs them, held until destroy
    unsigned *d_reject_map = nullptr;          // [npix] clipLow count | clipHigh count << 16 of the last maps pass
    bool last_maps = false;                    // the last pass was a maps pass: d_reject_map belongs to it
    uint16_t *d_coverage = nullptr;            // [npix]
    hipEvent_t ev_cov0 = nullptr, ev_cov1 = nullptr;       // around the kernels of the last nl_stack_coverage
    unsigned fb_hint = 0;                      // exact-list length of the last finished fast pass + 1 (0 = unknown)
    unsigned gen_hint = 0;                     // same for the generic list
    bool last_weighted = false;                // the last pass ran with weights (key of the hints it leaves)
    PassFacts last;                            // what the last pass left behind (all false after a failed one)
    unsigned dev_flags = 0;                    // nl_stack_set_dev_flags (A/B measurements)
    unsigned *d_fb_list = nullptr;             // [npix] pixels the fast kernel handed to the exact kernel
    unsigned *d_fb_count = nullptr;            // [2]: exact-list length, generic-list length (inside d_partial)
    unsigned *d_gen_list = nullptr;            // [npix] pixels zonal waves handed to the generic pass
    bool force_exact = false;
    int exact_flavour = 0;            // nl_stack_set_exact argument: 1 = LDS column kernel, 2 = wave-per-pixel replay
    unsigned long long *d_counters = nullptr;  // [4]: where a pass leaves {clip_low, clip_high, list lengths, -}: the handle's own buffer or the caller's (nl_stack_set_counters_buffer)
    unsigned long long *d_counters_own = nullptr;
    double *d_stat_partial = nullptr;          // [kStatBlocks*3]
    // linear-fit cascade (stack_linfit.hip): ping-pong pixel lists + liveness masks, lazily allocated
    unsigned *d_lf_list[2] = {nullptr, nullptr};
    uint4 *d_lf_state[2] = {nullptr, nullptr};
    unsigned *d_lf_count = nullptr;
    int lf_lanes = 0;                          // liveness masks per listed pixel the state arrays were sized for
    bool lf_tried = false;
    nl::DevBuffer ingest;                      // raw FITS bytes / unaligned source frame
    // asynchronous uploads: pinned staging ring + copy stream (nl_stack_upload_frame_async)
    hipStream_t copy_stream = nullptr;
    size_t stage_cap[kStageSlots] = {0, 0, 0, 0};
    nl::DevBuffer ingest_async;                // raw bytes / source frame of the overlapped ingest (copy stream)
    double *d_stat_partial_async = nullptr;
    void *h_stage[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t stage_done[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
    bool stage_used[kStageSlots] = {false, false, false, false};
    int stage_next = 0;
    bool uploads_pending = false;
    // scratch of the steps on one resident frame (nlstack_frame*.hip), lazily allocated
    struct FrameScratch {
        // bad-pixel step (nl_stack_frame_badpixel): diff, per-workgroup lists, ordered list (parked between handles);
        // nl::BpParams + per-workgroup list lengths, offsets, bad-pixel counts
        nl::ParkedBuffer bp_diff, bp_seg, bp_list;
        nl::DevBuffer bp_small;
        // colour-camera front (nl_stack_upload_frame_cfa): the raw mosaic, the compact delta / median of one
        // channel, row sums, per-workgroup counts, nl::BayerParams
        nl::DevBuffer cfa;
        // star detection (nl_stack_frame_find_stars / nl_stack_result_find_stars)
        nl::StarWork star_work;
        // background extraction (nl_stack_frame_back_extract)
        nl::BackWork back_work;
        // debanding (nl_stack_frame_deband_horiz / _vert)
        nl::DebandWork deband_work;
        // Gaussian blur / unsharp mask (nl_stack_frame_gaussian_blur, nl_stack_result_unsharp_mask, ...)
        nl::BlurWork blur_work;
        // the tone curves with statistics (nl_stack_frame_tone, ...): the transformed element 0, one float
        nl::DevBuffer tone_seed;
        // the colour steps (nl_stack_rgb_*): partials and seeds of three planes, block means, stars and their sums
        nl::ColourWork colour_work;
        // location and scale (nl_stack_frame_location_scale)
        nl::LocScaleWork locscale_work;
        size_t bytes() const
        {
            return bp_diff.bytes + bp_seg.bytes + bp_list.bytes + bp_small.bytes + cfa.bytes + star_work.bytes() +
                   back_work.bytes() + deband_work.bytes() + blur_work.bytes() + tone_seed.bytes + colour_work.bytes() +
                   locscale_work.bytes();
        }
        void release(int device)
        {
            bp_diff.release(device);
            bp_seg.release(device);
            bp_list.release(device);
            bp_small.release();
            cfa.release();
            star_work.release();
            back_work.release();
            deband_work.release();
            blur_work.release();
            tone_seed.release();
            colour_work.release();
            locscale_work.release();
        }
    } frame_scratch;
    int max_grid = 0;
    int last_mode = -1;
    bool pending = false;
    const char *last_kernel = "";
};

// developer switches of the projection (nl_stack_set_dev_flags; the others: nlstack_pass.hip) as launch_project takes them
constexpr unsigned kDevProjectDirect = 32768u;       // no tile stages its source box in LDS
constexpr unsigned kDevProjectPlainStores = 65536u;  // plain instead of nontemporal result stores
constexpr unsigned kDevColourDirect = 131072u;       // the darkest-block means stage no strip in LDS
constexpr unsigned kDevSquareEveryCandidate = 262144u;  // the square drizzle evaluates the edges of every candidate
inline unsigned project_switches(const nl_stack *h)
{
    return ((h->dev_flags & kDevProjectDirect) ? nl::kProjDirectOnly : 0u) |
           ((h->dev_flags & kDevProjectPlainStores) ? nl::kProjPlainStores : 0u);
}

#define NL_CHECK_HANDLE(h)                                              \
    do {                                                                \
        if (!(h)) return fail(NL_ERR_INVALID_ARG, "null handle");       \
        NL_HIP(hipSetDevice((h)->device));                              \
    } while (0)

// entry points that read frames on h->stream outside a stack pass first let pending
// asynchronous uploads land
#define NL_SETTLE_UPLOADS(h)                                            \
    do {                                                                \
        if ((h)->uploads_pending) {                                     \
            NL_HIP(hipStreamSynchronize((h)->copy_stream));             \
            (h)->uploads_pending = false;                               \
        }                                                               \
    } while (0)
