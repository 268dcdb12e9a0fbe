// stack_kernels.h -- shared declarations of libnlstack's HIP kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/nlstack.h"

// Result stores of the streaming kernels are NONTEMPORAL (round 6): the one store per pixel a stack pass makes is
// what the slow allocations of section 11.9 are slow beside -- reads + plain stores 6.12 against 6.77 TB/s, reads + nontemporal
// stores 6.52 against 6.93 (tools/ubench/alloc_probe_modes.hip): +2.4 % on every frame buffer, +6.5 % on the unlucky ones.
// NL_PLAIN_STORES (build switch) restores plain stores for A/B libraries.
#if defined(__HIPCC__)
#ifdef NL_PLAIN_STORES
#define NL_STORE_RESULT(ptr, val) (*(ptr) = (val))
#else
#define NL_STORE_RESULT(ptr, val) __builtin_nontemporal_store((val), (ptr))
#endif
#endif

namespace nl {

// 160 KiB LDS per CU (MI355X); a single workgroup may use all of it.
constexpr size_t kLdsBudgetBytes = 160 * 1024;
// clip counters: sharded accumulators [kClipSlots][2], zeroed before every pass
constexpr int kClipSlots = 256;

struct StackArgs {
    const float *frames;          // planar [n_frames][stride] fp32
    int64_t stride;               // floats between consecutive frames (>= tile pixels: the owned buffer is padded, nlstack_api.hip padded_frame_stride)
    int64_t npix;                 // pixels in the tile
    int64_t tiles;                // work items (wave tiles) in the launch
    int n_frames;
    int n_pad;                    // next power of two >= n_frames (sorting modes)
    const float *weights;         // device, n_frames floats, or nullptr
    const float *xstat;           // device, [n_frames+1][2]: MeanStdDev of 0..n-1 (linear fit)
    float sig_lo, sig_hi, ref_loc;
    float *out;                   // [npix]
    unsigned long long *partial;  // [kClipSlots][2] sharded clip counters (atomic adds)
    const unsigned *list;         // optional: pixel indices to process instead of 0..npix-1
    const unsigned *list_count;   // device-side length of `list`
    unsigned list_capacity;
    // wave-per-pixel replay only: a cell (zero before the pass) shared by the two replays of a pass.  The
    // first workgroup of either to look stores 1 + the list's length at that moment; part 0 replays the
    // items before that snapshot (what the dominant kernel handed over), part 1 the items from it on
    // (what the generic pass added) -- no host-enqueued snapshot copy between the kernels
    unsigned *list_snap;
    int list_part;
    // Fused pass protocol of the sigma / winsorized fast path (nlstack_api.hip): no memset before and no
    // reduction kernel after a pass.  The dominant kernel's first workgroup zeroes `final` and the scratch set
    // of the NEXT pass (`zero_next`, kScratchWords words: the sets alternate); the dominant kernel adds its
    // clip counts to this pass's sharded `partial` slots; the first workgroup of the generic pass sums them
    // into `final`; every kernel after the dominant one (generic pass, replays) adds to `final` directly.
    // The replays add to one address, which is only cheap while their lists are short (thousands of workgroups
    // adding to one word take longer than a reduction kernel): nlstack_api.hip runs a pass fused only if the last
    // finished pass reported a short exact list.  All nullptr: the plain protocol (memset, sharded slots,
    // reduce_counters_kernel).
    unsigned long long *final;    // [2] clip totals of the pass
    unsigned long long *zero_next;
    // Weighted stacks, decision pass + permutation replay (stack_fast_decide.hip): thresholds that reproduce the
    // reference's clip decisions, [round][pixel] (round stride = npix), and the number of rounds per pixel (0 = not
    // decided: the replay computes its own bounds, as without these).  nullptr: off.
    float2 *bounds;
    unsigned char *nrounds;
    // Maps pass (nl_stack_run_maps and the tiers above it): [npix] words, the pixel's clipLow
    // count | clipHigh count << 16.  Read by the MAPS instantiations only (stack_exact_kernel; stack_fast_maps_impl.hpp;
    // stack_linfit_impl.hpp; the MAD kernels of stack_fast.hip / stack_fast_ml.hip / stack_fast_ml_deep.hip; coop_body);
    // nullptr everywhere else.
    unsigned *reject_map;
};

// words (64 bit) of one per-pass scratch set: clip accumulators + {exact-list length, generic-list length,
// list snapshot, spare} (32 bit each)
constexpr int kScratchWords = 2 * kClipSlots + 2;

// fallback list written by the fast kernels, consumed by the exact kernel
struct FastArgs {
    unsigned *fb_list;            // [fb_capacity] pixels for the exact kernel
    unsigned *fb_count;           // device counter, zeroed before every pass
    unsigned fb_capacity;
    unsigned *fb_snap;            // optional, see StackArgs::list_snap: a generic pass stores 1 + *fb_count here before it appends
    unsigned *gen_list;           // [gen_capacity] pixels a zonal wave hands to the generic pass
    unsigned *gen_count;          // device counter, zeroed before every pass
    unsigned gen_capacity;
    unsigned gen_hint;            // 1 + the generic list's length in the last finished pass (0 = unknown): sizes the generic grid
    const unsigned *in_list;      // generic pass: list to process (nullptr = the whole tile)
    const unsigned *in_count;
    unsigned in_capacity;
    // Winsorization cascade of the one-lane winsorized kernels (stack_fast_sigma_impl.hpp).  Host-side plan, filled in by
    // nlstack_api.hip: two continuation lists (pixel, clip counts so far) with their per-workgroup lengths and the wave
    // budgets of the first two stages (winsorization rounds; the third stage runs to the end).  cas_list[0] == nullptr:
    // no cascade.  NO global atomics: a workgroup of a stage compacts its unfinished pixels into a region of its own
    // (through an LDS counter) and stores the region's length; a workgroup of the next stage takes cas_group consecutive
    // regions.  (One device counter for the 262 144 waves of a 4096^2 tile costs 3 ms -- 11 ns per atomic, all in one L2
    // channel -- whether it is one word or 256 neighbouring ones: measured, the dominant kernel got slower with a budget.)
    // Stage k (0 = the dominant kernel) appends to list k % 2 and, from k = 1 on, reads list (k - 1) % 2; it may run
    // cas_pass[k] clipping passes per wave with at most cas_cap[k] winsorization rounds each (0 = no limit: the last stage).
    unsigned *cas_list[2];
    unsigned *cas_state[2];
    unsigned *cas_count[2];       // lengths of the regions of the two lists (one region per workgroup of the stage that filled it)
    int cas_stages;               // stages in all, 2 ... kCascadeStages
    int cas_pass[6], cas_cap[6];
    int cas_group[6];             // [k]: regions of its input list per workgroup of stage k (k >= 1), at most 16
    // ... and what one launch of the cascade works with (set by the launcher from the plan above)
    unsigned *cont_list;          // where this stage appends its unfinished pixels: region blockIdx.x, cont_region entries long
    unsigned *cont_state;
    unsigned *cont_count;         // [workgroups of this launch]
    unsigned cont_region;
    const unsigned *in_state;     // CONT kernels: the states that belong to in_list; in_count = the regions' lengths
    unsigned in_region, in_regions, in_group;      // entries per input region, number of regions, regions per workgroup
    int pass_budget, round_cap;   // clipping passes a wave may run in this stage / winsorization rounds per pass (0 = no limit)
    int record_only = 0;          // LDS-column kernels as the DECISION pass of a weighted stack (129 ... 512 frames): no outputs, no
                                  // lists, no counters -- only StackArgs::bounds / nrounds (0 rounds for a pixel they would hand over).
                                  // Set by launch_stack_sigma_mlz for Form::Record, by nobody else
    int cert_first = 0, cert_every = 1;      // invariant-interval certificate of the winsorization loops (stack_fast_sigma_impl.hpp): first trial after this many rounds of a loop (0: off), then every so many
    int gen_round_cap = 0;        // generic pass of the one-lane winsorized kernels: winsorization rounds per clipping pass before a pixel
                                  // is handed to the exact replay instead (0: 100, the limit of every kernel)
};

// The FORM of a stack kernel: what an instantiation does beside, or instead of, its plain work.  Every launcher that
// has forms takes one `Form form = Form::Plain` and returns hipErrorInvalidValue for a form it has no instantiation of,
// or whose StackArgs fields are missing (form_args_ok).  On the device the forms are the bool template parameters MAPS,
// FOLLOW and RECORD.
//   Plain   the kernel as every default pass runs it;
//   Maps    also store the pixel's two clip counts, clipLow | clipHigh << 16 (a maps pass): needs args.reject_map;
//   Follow  weights follow their frames (the weighted clip and MAD-sigma passes): needs args.weights;
//   Record  leave only the clip bounds, no outputs, lists or counters (a decision pass): needs args.bounds and
//           args.nrounds.
enum class Form { Plain, Maps, Follow, Record };
inline bool form_args_ok(Form form, const StackArgs &args)
{
    switch (form) {
    case Form::Maps:   return args.reject_map != nullptr;
    case Form::Follow: return args.weights != nullptr;
    case Form::Record: return args.bounds != nullptr && args.nrounds != nullptr;
    default:           return true;
    }
}

// sets what nl_last_error() returns on this thread (nlstack_api.hip)
void set_last_error(const char *msg);
// nl_stack_frame_project_from / nl_group_frame_project_from and, with a kernel (NL_RS_*, checked by the caller) and the
// clamp, their _resample_from forms (nlstack_frame.hip, with nl::stack_settle); who = the call's name in messages
int stack_project_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, const float trans[6],
                       float out_of_bounds, const char *who, bool from_group, int kernel = NL_RS_BILINEAR, int clamp = 0);
// what the _resample_from entries check in front of their handles: the kernel's id, a null or singular transform
int resample_args_check(const char *who, int kernel, const float *trans);
int stack_settle(nl_stack_t *h);

// ---- stack_exact.hip ----
// Picks lanes-per-wave and LDS bytes for the exact kernel; -1 if it cannot fit.
int exact_plan(int mode, bool weighted, int n_frames, int n_pad, int max_lanes, int *lanes,
               size_t *lds_bytes);
// Plain, Maps or Follow, over the whole tile or -- the replay behind the other kernels of a pass -- the pixels of args.list.
// The median, MAD sigma and a Maps linear fit drop `weighted`.  Follow (the weighted clip pass, include/nlstack_wclip.h:
// NL_ST_SIGMA / NL_ST_WINSOR_SIGMA, one column; the weighted MAD-sigma pass: two columns) ignores it: plan with weighted = false
hipError_t launch_stack_exact(int mode, bool weighted, const StackArgs &args, int lanes, int grid,
                              size_t lds_bytes, hipStream_t stream, const char **name, Form form = Form::Plain);
// list_counts (optional): {exact-list length, generic-list length} of the pass, left in counters[2] (low | high << 32)
// zero_after: the kernel leaves the scratch set (kScratchWords words at `partial`) zeroed for the next pass
hipError_t launch_reduce_counters(unsigned long long *partial, int n_blocks,
                                  unsigned long long *counters, hipStream_t stream,
                                  const unsigned *list_counts = nullptr, bool zero_after = false);

// ---- stack_fast.hip ----
// one-lane register kernels address a group of 4 frames through one buffer descriptor with
// 32-bit offsets (3 frames + the pixel): tiles of 2^27 pixels or more take the int64-indexed kernels
constexpr int64_t kFastMaxPixels = (int64_t)1 << 27;
int fast_supported(int mode, bool weighted, int n_frames, int64_t npix);
hipError_t launch_stack_median_fast(const StackArgs &args, const FastArgs &fargs, hipStream_t stream,
                                    const char **name, hipEvent_t dominant_done);
// dominant_done (optional) is recorded right after the first, dominant kernel
int mad_fast_supported(int mode, bool weighted, int n_frames, int64_t npix);
// Plain, Follow (the weighted MAD-sigma pass, include/nlstack_wmad.h) or Maps (the full maps pass, include/nlstack_fullmaps.h)
hipError_t launch_stack_mad_fast(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                 Form form = Form::Plain);
// 249..256 / 505..512 frames: zonal sigma / winsorized sigma pass with the clipping rounds on LDS
// columns (stack_fast_mlz.hip); hand-over lists as the other fast kernels
// generic pass of the multi-lane sigma / winsor kernels over fargs.in_list, whole columns in LDS (stack_fast_mlg.hip)
// Maps (both launches, 129 ... 512 frames: the two parts of a maps pass at that depth): stack_fast_mlz_maps_{a,b,c,d}.hip,
// stack_fast_mlg.hip.  launch_stack_sigma_mlz also takes Record (the decision pass of a weighted stack): the launcher then
// passes the kernel a FastArgs of its own, all zero but record_only = 1, whatever `fargs` holds
hipError_t launch_stack_sigma_mlg(const StackArgs &args, const FastArgs &fargs, unsigned grid, hipStream_t stream,
                                  bool winsor, Form form = Form::Plain);
int fast_mlz_supported(int mode, bool weighted, int n_frames);
hipError_t launch_stack_sigma_mlz(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                  bool winsor, Form form = Form::Plain);
// sigma / winsorized clipping of 2 ... 128 frames, in the two parts a pass enqueues them.  Dominant part: the zonal kernel
// (network size 8: the generic kernel over the whole tile), dominant_done (optional) recorded behind it, and for winsorized
// stacks the continuation stages of the cascade.  Generic part: the pass over the generic list (network size 8: nothing);
// with first_replay (tail_fused_supported) it shares ONE launch with the replay of the exact list as the dominant part left
// it (stack_tail_fused.hip) -- *first_replay are that replay's arguments (list part 0), in replay_blocks workgroups
// Maps (stack_fast_maps_sigma.hip / stack_fast_maps_winsor.hip): as the parts above with one more store per pixel; no cascade
// plan in fargs, no first_replay, no hints -- the generic part runs a fixed grid
hipError_t launch_stack_sigma_dominant(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                       hipEvent_t dominant_done, bool winsor, Form form = Form::Plain);
hipError_t launch_stack_sigma_generic(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, bool winsor,
                                      Form form = Form::Plain, const StackArgs *first_replay = nullptr, unsigned replay_blocks = 0);
// ---- stack_tail_fused.hip: generic pass (one lane per pixel, LDS columns) + first replay in one grid; plain sigma, 65 ... 128 frames
int tail_fused_supported(int mode, bool weighted, int n_frames);
hipError_t launch_stack_sigma_tail(const StackArgs &generic, const FastArgs &fargs, unsigned gen_blocks,
                                   const StackArgs &replay, unsigned replay_blocks, hipStream_t stream);

constexpr int kCascadeStages = 6;   // most stages of a winsorization cascade, the dominant kernel included
// rounds of clip bounds a decision pass records per pixel (pixels that need more are replayed in full)
constexpr int kBoundRounds = 8;
// ---- stack_fast_decide.hip: the register-resident kernels as the DECISION pass of weighted sigma / winsorized
// stacks (StackArgs::bounds / nrounds); 33 ... 128 frames (decide_supported); 129 ... 512 frames: the LDS-column kernel
// of the frame-count class, record-only (decide_ml_supported) ----
int decide_supported(int mode, int n_frames, int64_t npix);
int decide_ml_supported(int mode, int n_frames, int64_t npix);      // 129 ... 512 frames: launch_stack_sigma_mlz, Form::Record
hipError_t launch_stack_sigma_decide(const StackArgs &args, hipStream_t stream, bool winsor, const char **name);

// ---- stack_fast_ml.hip (129..512 frames, 2 or 4 lanes per pixel) ----
constexpr int kMlNS = 128;     // samples per lane of the multi-lane kernels
int fast_ml_supported(int mode, bool weighted, int n_frames, int64_t npix);
hipError_t launch_stack_median_ml(const StackArgs &args, hipStream_t stream, const char **name);
// Plain, Maps (the full maps pass) or Record (the weighted MAD-sigma pass: one round per pixel, `fargs` is not read)
hipError_t launch_stack_mad_ml(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                               Form form = Form::Plain);
unsigned ml_generic_grid(int n_frames, unsigned gen_hint);      // workgroups of launch_stack_sigma_mlg behind launch_stack_sigma_mlz

// the same two kernels on 8 / 16 lanes per pixel: the median and unweighted MAD sigma of 513 ... 2048 frames
// (stack_fast_ml_deep.hip; include/nlstack_deepstack.h).  `stride`: floats between frames, LPP * stride * 4 < 2^31
// The MAD kernel: Plain, Maps (include/nlstack_deepstackmaps.h) or Record (include/nlstack_deepwmad.h), as launch_stack_mad_ml
int deep_ml_supported(int mode, bool weighted, int n_frames, int64_t stride);
hipError_t launch_stack_median_ml_deep(const StackArgs &args, hipStream_t stream, const char **name);
hipError_t launch_stack_mad_ml_deep(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                    Form form = Form::Plain);

// ---- stack_exact_coop.hip (bit-exact sigma replay, one wave per pixel) ----
int coop_supported(int mode, bool weighted, int n_frames);
hipError_t launch_stack_median_coop(const StackArgs &args, int grid, hipStream_t stream, const char **name);
// Plain, or Maps (include/nlstack_deepstackmaps.h): the whole-tile, unweighted replay only -- refused with weights or a list
hipError_t launch_stack_sigma_coop(int mode, const StackArgs &args, int grid, hipStream_t stream, const char **name,
                                   Form form = Form::Plain);
int coop_group(const StackArgs &args);      // pixels per work item of that launch (4: whole-tile replay with aligned 16-byte loads)

// ---- stack_exact_tile.hip (bit-exact sigma / winsorized clipping over whole tiles: one wave = 64
// consecutive pixels, columns in LDS, one pixel per lane; the weighted modes' default path) ----
// frame counts up to which it beats the other replays over a whole tile (tools/replay_probe2.py, weighted stacks,
// ms per 512 x 4096 pixels, tile / four pixels per wave / one pixel per wave -- sigma: 40 frames 1.54 / 2.16 / 2.79,
// 56 frames 2.82 / 2.84 / 3.17, 64 frames 3.5 / 2.9 / 3.2; winsorized: 40 frames 4.37 / 5.22 / 8.11, 48 frames
// 5.34 / 5.28 / 8.25, 56 frames 6.70 / 6.27 / 8.54)
constexpr int kTileMaxFramesSigma = 40, kTileMaxFramesWinsor = 32;
// (those numbers are from before the decision pass.  With it -- 33 ... 128 frames: the register-resident kernel decides
// every round, the replay only permutes -- the one-pixel-per-wave replay needs no sequential sums any more and, with
// its partition passes in registers, wins wherever the decision pass exists, whole 4096^2 images in ms: sigma 36
// frames 9.3 (tile) vs 11.5, 44: 13.7 vs 13.7, 56: 21.7 vs 16.9, 64: 21.2 (four pixels per wave) vs 18.9, 96: 30.6
// vs 26.0; winsorized 36 frames 27.2 (tile) vs 16.6, 44: 36.2 vs 17.4, 96: 35.5 (four) vs 28.9, 128: 52.6 vs 38.3;
// with four pixels per work item (stack_exact_coop.hip, GROUP): sigma 34 frames 8.5 (tile) vs 11.1, 40: 11.4 vs 11.7,
// 44: 13.7 vs 12.0.)
int tile_supported(int mode, bool weighted, int n_frames);
hipError_t launch_stack_sigma_tile(int mode, const StackArgs &args, int grid, hipStream_t stream, const char **name);

// ---- stack_linfit.hip (register-resident linear fit, bit-exact) ----
// Cascade: a stage runs at most max_iters fit iterations; pixels that are not done are
// appended to out_list together with their liveness mask (4 words) and continued by the
// next stage in freshly packed waves (lists and states: npix entries each).
struct LinfitCascade {
    unsigned *list[2];            // ping-pong pixel lists
    uint4 *state[2];              // liveness masks of the listed pixels
    unsigned *count;              // device: [kLinfitStages] list lengths, zeroed per pass
    unsigned capacity;
};
constexpr int kLinfitStages = 4;
constexpr int kLinfitCounters = 8;  // device list lengths of one pass (the bit-exact cascade uses the first kLinfitStages)
int linfit_fast_supported(int mode, int n_frames, int64_t npix);
int linfit_ml_supported(int mode, int n_frames, int64_t npix);

// Form::Maps: the MAPS instantiations of the same kernels (stack_linfit_maps.hip).  Same classes, cascade,
// quotas and grids; every lane that holds a pixel's two clip counts leaves them in args.reject_map (stage 0 stores,
// continuation stages add: stack_linfit_impl.hpp)
hipError_t launch_stack_linfit_fast(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                    hipStream_t stream, const char **name, hipEvent_t dominant_done, Form form = Form::Plain);
hipError_t launch_stack_linfit_ml(const StackArgs &args, const FastArgs &fargs, const LinfitCascade *cascade,
                                  hipStream_t stream, const char **name, hipEvent_t dominant_done, Form form = Form::Plain);

// ---- stack_linfit_weighted.hip (the weighted linear-fit pass, include/nlstack_wlinfit.h: register-resident fit, one
// pixel per lane, up to 128 frames; args.weights must be set; pixels it cannot decide go to fargs.fb_list, for
// launch_stack_exact(NL_ST_LINEAR_FIT, weighted = true, ...)) ----
int linfit_weighted_supported(int n_frames, int64_t npix);
hipError_t launch_stack_linfit_weighted(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name);

// ---- the weighted clip pass whose weights follow their frames (include/nlstack_wclip.h, an extension) ----
// stack_fast_decide_shallow.hip: the decision pass at 9 ... 32 frames (RECORD instantiations at network sizes 16 / 24 / 32);
// this pass only -- decide_supported and the weighted default pass stay at 33 frames
int decide_shallow_supported(int mode, int n_frames, int64_t npix);
hipError_t launch_stack_sigma_decide_shallow(const StackArgs &args, hipStream_t stream, bool winsor, const char **name);
// stack_clip_weighted.hip: one streaming read of the frames under the thresholds in args.bounds / args.nrounds, the
// weights from args.weights; pixels without a complete record go to fargs.fb_list, for launch_stack_exact(Form::Follow)
// one_round: the instantiations for which one recorded round is a complete record (the weighted MAD-sigma pass,
// include/nlstack_wmad.h, behind launch_stack_mad_ml(Form::Record))
hipError_t launch_stack_clip_weighted(const StackArgs &args, const FastArgs &fargs, hipStream_t stream, const char **name,
                                      bool one_round = false);

// ---- stack_mean.hip ----
hipError_t launch_stack_mean(bool weighted, const StackArgs &args, hipStream_t stream,
                             const char **name);
hipError_t launch_axpy(float *acc, const float *x, float weight, int first, int64_t n,
                       hipStream_t stream);
hipError_t launch_scale(float *acc, float factor, int64_t n, hipStream_t stream);

// ---- stack_coverage.hip: out[p] = frames whose sample at p is not NaN (the n of the gather, stack.go:380-387) ----
hipError_t launch_stack_coverage(const float *frames, int64_t stride, int64_t npix, int n_frames, uint16_t *out,
                                 hipStream_t stream);

// ---- ingest.hip (FITS payload decode / encode, MatchHistogram, Project from a frame that was just uploaded) ----
int fits_bytes_per_value(int bitpix);
hipError_t launch_fits_decode(const void *raw, int bitpix, int64_t n, float bscale, float bzero, bool affine,
                              float mult, float off, float *out, double *partial /*[blocks][3]*/, int blocks,
                              hipStream_t stream);
hipError_t launch_fits_encode(const float *data, int64_t n, int replace_nans, void *raw, hipStream_t stream);
hipError_t launch_affine(float *data, int64_t n, float mult, float off, hipStream_t stream);
hipError_t launch_project(const float *src, int src_w, int src_h, float *dst, int dst_w, int row0, int rows,
                          const float inv[6], float oob, bool affine, float mult, float off,
                          hipStream_t stream);

// ---- project.hip (Project from a resident frame; switches: kProjDirectOnly | kProjPlainStores of project.hpp) ----
hipError_t launch_project_tiled(const float *src, int src_w, int src_h, float *dst, int dst_w, int row0, int rows,
                                const float inv[6], float oob, unsigned switches, hipStream_t stream);
// how many tiles of that launch stage their source box in LDS, how many tap global memory (host arithmetic, the kernel's own)
void project_tile_paths(const float *src, int src_w, int src_h, int dst_w, int row0, int rows, const float inv[6],
                        unsigned switches, int64_t *staged, int64_t *direct);

// ---- resample.hip (the same projection with a bicubic or Lanczos-3 kernel, include/nlstack_resample.h: an extension) ----
// radius = 2 (bicubic) or 3 (Lanczos-3, with table = lanczos3_table_device of the stream's device); switches as above
hipError_t launch_resample_tiled(const float *src, int src_w, int src_h, float *dst, int dst_w, int row0, int rows,
                                 const float inv[6], float oob, int radius, bool clamp, const float *table,
                                 unsigned switches, hipStream_t stream);
void resample_tile_paths(const float *src, int src_w, int src_h, int dst_w, int row0, int rows, const float inv[6],
                         int radius, unsigned switches, int64_t *staged, int64_t *direct);
// the NL_RS_PHASES x 6 Lanczos-3 table: built once on the host; one copy per device, made by the first call that asks
// for it (the caller has selected `device`), kept for the life of the library
const float *lanczos3_table_host();
hipError_t lanczos3_table_device(int device, const float **table);

// ---- synth.hip ----
hipError_t launch_fill_synthetic(float *frames, int64_t stride, int n_frames, int width,
                                 int height, int row0, int rows, uint64_t seed,
                                 hipStream_t stream);

// ---- frame_stats.hip ----
hipError_t launch_min_sum_max(const float *data, int64_t n, double *partial /*[blocks][3]*/,
                              int blocks, hipStream_t stream);
hipError_t launch_variance(const float *data, int64_t n, float mean, double *partial /*[blocks]*/,
                           int blocks, hipStream_t stream);
hipError_t launch_noise(const float *data, int width, int height, double *partial /*[blocks]*/,
                        int blocks, hipStream_t stream);
hipError_t launch_median3x3(const float *in, float *out, int width, int height,
                            hipStream_t stream);
constexpr int kMedianMaskMax = 32;
hipError_t launch_median_mask(const float *in, float *out, int64_t n, const int *mask, int len, hipStream_t stream);

}  // namespace nl
