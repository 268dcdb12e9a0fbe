/*
 * nlstack.h -- C ABI of libnlstack.so: MI355X (gfx950) implementation of
 * Nightlight's per-pixel stacking hot path.
 *
 * This is the drop-in boundary.  A thin cgo shim (go/ and INTEGRATION.md)
 * binds exactly these entry points from a replacement of the reference's
 * `internal/ops/stack` package, keeping the ops.Operator surface
 * (internal/ops/operator.go:135-138) and OpStack's JSON fields
 * (internal/ops/stack/stack.go:66-73) unchanged.
 *
 * Conventions
 *   - plain C types only; every pointer is caller-owned and is NOT retained
 *     after the call returns (cgo pointer rules), except device pointers the
 *     caller explicitly lends with nl_stack_attach_device_frames();
 *   - functions returning int return NL_OK (0) or a negative NL_ERR_* code and
 *     never abort; nl_last_error() gives the message of the calling thread's
 *     last failure (the Go shim turns it into an `error`);
 *   - every entry point selects its handle's device itself (goroutines migrate
 *     between OS threads; SURVEY.md section 8b "Threading");
 *   - stack modes are numbered exactly as StackMode, stack.go:33-42.
 *
 * Data layout in HBM: frames are planar [n_frames][rows*width] fp32 for the
 * row tile [row0, row0+rows) of a width x height image (whole image: row0=0,
 * rows=height).  NaN = "no data" (alignment out-of-bounds), as the reference.
 */
#ifndef NLSTACK_H
#define NLSTACK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* StackMode, internal/ops/stack/stack.go:33-42 */
#define NL_ST_MEDIAN        0
#define NL_ST_MEAN          1
#define NL_ST_SIGMA         2
#define NL_ST_WINSOR_SIGMA  3
#define NL_ST_MAD_SIGMA     4
#define NL_ST_LINEAR_FIT    5
#define NL_ST_AUTO          6

/* StackWeighting, internal/ops/stack/stack.go:57-63 */
#define NL_WEIGHT_NONE           0
#define NL_WEIGHT_EXPOSURE       1
#define NL_WEIGHT_INVERSE_NOISE  2
#define NL_WEIGHT_INVERSE_HFR    3

#define NL_OK                      0
#define NL_ERR_INVALID_MODE       -1  /* "invalid stacking mode", stack.go:119 */
#define NL_ERR_MISSING_EXPOSURE   -2  /* "%d: Missing exposure information ...", stack.go:238 */
#define NL_ERR_INVALID_WEIGHTING  -3  /* "Invalid weighting mode %d", stack.go:267 */
#define NL_ERR_WEIGHTED_MAD       -4  /* the reference panics (stack.go:185); we return an error */
#define NL_ERR_NO_INPUTS          -5  /* "stack operator needs inputs", stack.go:103 */
#define NL_ERR_INVALID_ARG        -6
#define NL_ERR_HIP                -7  /* HIP runtime failure; message has the hipError string */
#define NL_ERR_TOO_MANY_FRAMES    -8  /* per-pixel column does not fit the 160 KiB LDS */
#define NL_ERR_NO_DEVICE          -9

typedef struct nl_stack nl_stack_t;

/* message of the calling thread's last error ("" if none) */
const char *nl_last_error(void);
/* number of visible HIP devices, or a negative error */
int nl_device_count(void);
/* library version string.  0.2.0 (round 5 / 6): the OWNED frame buffer is padded -- frame k starts at
 * nl_stack_frames_device_ptr(h) + k * nl_stack_frame_stride(h) floats, NOT at k * rows * width; a producer written
 * against 0.1.0's dense layout must read the stride (or lend its own dense buffer with nl_stack_attach_device_frames). */
const char *nl_version(void);
/* nl_stack_destroy parks the large device buffers of a handle (frames, result, hand-over lists, the scratch of the
 * winsorized / linear-fit cascades and of weighted passes; per device at most 64 blocks and NL_MEM_CACHE_MB MiB -- default:
 * a sixteenth of the device's memory, 0 turns the cache off) for the next nl_stack_create / nl_group_create of the same
 * geometry on the same device: a drop-in that creates one handle per OpStack.Apply (stack.go:131-138 allocates per
 * call, too) otherwise pays more for hipMalloc + hipFree than for the stack pass.  This returns the parked buffers to
 * HIP.  The library does so itself whenever ANY of its own device allocations fails (every one of them goes through
 * one helper that releases the cache and retries); allocations of OTHER code in the process (torch, RCCL) do not see
 * the parked blocks as free memory -- call this, or set NL_MEM_CACHE_MB=0, when the process shares the device.
 * The streams of destroyed handles are parked the same way (main + side stream as the pair they were created as, copy
 * streams in a list of their own, up to 16 of each per device: destroying a handle's two or three streams was 0.5 ms of
 * its 0.55 ms, creating them 0.2 of 0.24; NL_STREAM_POOL=0 turns it off), and so are the pinned staging buffers of the
 * asynchronous uploads (at most 16 blocks / 2 GiB per process: hipHostMalloc + hipHostFree of the ring were 20 ms of an
 * Apply from host memory); all are released here as well.  The limits are per device (a sixteenth of THAT device's
 * memory); a buffer above the limit -- the 32 GiB frame buffer of a 512 x 4096 x 4096 stack -- is never parked.
 * No counterpart in the reference. */
void nl_release_cached_memory(void);

/* ---- handle: replaces the per-call state of OpStack.Apply (stack.go:115-227) ---- */

/* Allocates the planar [n_frames][rows*width] device buffer, the result tile
 * and the counter scratch on `device`.  Returns NULL on failure. */
nl_stack_t *nl_stack_create(int n_frames, int width, int height, int row0, int rows, int device);
void nl_stack_destroy(nl_stack_t *h);

/* Copies the handle's row tile out of one full host frame (width*height
 * floats = fits.Image.Data, internal/fits/fits.go:42) into slot `idx`.
 * Synchronous; the pointer is not retained.  One call per Go slice. */
int nl_stack_upload_frame(nl_stack_t *h, int idx, const float *host_frame);
/* Same, but the host buffer holds only the tile (rows*width floats). */
int nl_stack_upload_tile(nl_stack_t *h, int idx, const float *host_tile);
/* Overlapped upload (caller side of the path, OpStackBatches' frame loop,
 * internal/ops/stack/stackbatches.go:68-96): the frame's tile is copied into a
 * pinned staging buffer and the call returns -- host_frame is not retained --
 * while the DMA proceeds on a copy stream.  The next nl_stack_run* waits for
 * the uploads on the device; nl_stack_upload_wait waits on the host. */
int nl_stack_upload_frame_async(nl_stack_t *h, int idx, const float *host_frame);
int nl_stack_upload_wait(nl_stack_t *h);
/* Device address of the planar frame buffer (for in-place producers that
 * already live on the GPU); valid until destroy/attach.  Frame k starts at
 * nl_stack_frame_stride(h) * k floats, see below. */
void *nl_stack_frames_device_ptr(nl_stack_t *h);
/* ---- FITS framing (host): where the payload sits in a file image, and the frame around a result ------------------
 * internal/fits/read.go:445-469 reads the header in 2880-byte units of 80-byte cards up to END; :97-147 take SIMPLE,
 * BITPIX, NAXIS, NAXISn (mandatory) and BZERO (default 0), BSCALE (default 1), EXPOSURE or else EXPTIME (default 0) from
 * it.  internal/fits/write.go:54-89 writes SIMPLE, BITPIX -32, NAXIS, NAXISn, BZERO, BSCALE, EXPOSURE (if non-zero),
 * PROGRAM, END, pads header and payload to 2880 bytes with spaces.  The payload itself is decoded / encoded on the device
 * (nl_stack_upload_frame_fits, nl_stack_download_result_fits). */
#define NL_FITS_MAX_AXES 8
typedef struct nl_fits_header {
    int32_t bitpix, naxis, naxisn[NL_FITS_MAX_AXES];
    float bzero, bscale, exposure;
    int64_t pixels;                  /* product of the axes */
    int64_t header_bytes;            /* = offset of the payload in the file, a multiple of 2880 */
    int64_t payload_bytes;           /* pixels * |bitpix| / 8 */
    int64_t padded_payload_bytes;    /* the same, rounded up to 2880 */
} nl_fits_header_t;
/* parses the header at the start of a file image; `id` is the frame number the reference puts in front of its messages */
int nl_fits_parse_header(const void *file_bytes, int64_t n_bytes, int id, nl_fits_header_t *out);
/* the header Image.Write emits for a BITPIX -32 image; returns its length (a multiple of 2880; with dst == NULL only
 * that), -1 on error */
int64_t nl_fits_write_header(void *dst, int64_t capacity, int naxis, const int32_t *naxisn, float bzero, float bscale,
                             float exposure);
int64_t nl_fits_padded_bytes(int64_t payload_bytes);

/* Device memory (bytes) the handle holds right now: the buffers of nl_stack_create plus what passes and upload paths
 * have allocated since and keep until nl_stack_destroy (e.g. 65 bytes per pixel of the tile for the thresholds of the
 * weighted clip modes' decision pass).  The reference sizes its batches to host memory (stackbatches.go:121-187); a
 * caller doing the same for the device reads this.  No counterpart in the reference. */
int64_t nl_stack_device_bytes(nl_stack_t *h);
/* Lends an existing DENSE device buffer -- frame k at device_frames + k * rows * width floats -- instead of the
 * owned one (NULL restores the owned buffer).  The caller keeps it alive. */
int nl_stack_attach_device_frames(nl_stack_t *h, void *device_frames);
/* Frame layout.  The owned buffer is planar with nl_stack_frame_stride(h) floats between consecutive frames:
 * rows*width rounded up, plus a fixed padding, so that the same pixel of consecutive frames does not fall into the
 * same HBM channel and bank (a power-of-two frame size such as 4096 x 4096 x 4 bytes otherwise costs the 512-frame
 * pass 12 %).  Producers that write through nl_stack_frames_device_ptr, and handles that
 * borrow another handle's frames, use this stride: frame k starts at ptr + k * stride floats.  The _strided attach
 * lends a buffer of any stride >= rows*width (a multiple of 4 floats when rows*width is one); the plain attach above
 * is the stride rows*width.  All upload / download / ingest / statistics entry points follow the handle's current
 * stride.  No counterpart in the reference (its frames are separate Go slices). */
int64_t nl_stack_frame_stride(nl_stack_t *h);
int nl_stack_attach_device_frames_strided(nl_stack_t *h, void *device_frames, int64_t frame_stride);
/* Fills all frames on the device with the deterministic synthetic stack of
 * SURVEY.md section 8d (sky gradient + per-frame gain/offset/noise, 0.4 % hot
 * and 0.1 % cold outliers, NaN borders, one all-NaN 8x8 patch).  Pixel
 * coordinates are those of the full image, so tiles agree with the whole. */
int nl_stack_fill_synthetic(nl_stack_t *h, uint64_t seed);
/* Downloads frame `idx`'s tile (rows*width floats). */
int nl_stack_download_tile(nl_stack_t *h, int idx, float *host_tile);
/* Downloads n_rows rows starting at tile-relative row first_row (n_rows*width
 * floats) of frame `idx`, or of the result tile of the last finished pass when
 * idx == -1.  Rows are contiguous in the planar layout, so this is one DMA;
 * it lets a caller inspect parts of stacks far larger than host memory. */
int nl_stack_download_rows(nl_stack_t *h, int idx, int first_row, int n_rows, float *host_rows);

/* Frames in use by the next uploads / passes: slots [0, n), 1 <= n <= the n_frames given
 * to nl_stack_create.  Lets a batch loop (OpStackBatches, stackbatches.go:69-111) keep one
 * handle and its device accumulator across batches of different sizes.  Clears the weights
 * when n changes. */
int nl_stack_set_active_frames(nl_stack_t *h, int n);
/* getWeights (stack.go:231-270).  weights: n_frames floats or NULL = none. */
int nl_stack_set_weights(nl_stack_t *h, const float *weights);
/* Computes the weights from per-frame scalars exactly as getWeights does:
 * NL_WEIGHT_EXPOSURE: w=exposure (error if 0, *bad_index = frame);
 * NL_WEIGHT_INVERSE_NOISE / _HFR: w = 1/(1+4*(v-min)/(max-min)).
 * Pure host arithmetic, no device work. */
int nl_weights_from_scalars(int weighting, const float *per_frame, int n_frames,
                            float *weights_out, int *bad_index);

/* One stack pass = the numeric core of OpStack.Apply (stack.go:142-218):
 * runs Stack{Median,Mean,MeanWeighted,Sigma,SigmaWeighted,MADSigma,
 * WinsorSigma,WinsorSigmaWeighted,LinearFit} (stack.go:274-918) over the tile.
 * mode NL_ST_AUTO is resolved from n_frames as stack.go:45-55.
 * out_host: full-image buffer (width*height floats); the tile's rows are
 * written at offset row0*width.  NULL leaves the result on the device.
 * clip_low/high: totals for THIS tile (sum them across tiles/ranks). */
int nl_stack_run(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                 float *out_host, int64_t *clip_low, int64_t *clip_high);
/* Asynchronous split of the same: enqueue on the handle's stream ... */
int nl_stack_run_async(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc);
/* ... then wait and fetch.  Any of the three outputs may be NULL. */
int nl_stack_finish(nl_stack_t *h, float *out_host, int64_t *clip_low, int64_t *clip_high);
/* Device address of the result tile (rows*width floats). */
void *nl_stack_result_device_ptr(nl_stack_t *h);
/* Mode actually run by the last pass (after NL_ST_AUTO resolution). */
int nl_stack_last_mode(nl_stack_t *h);
/* GPU time of the last pass's kernels in ms, from HIP events recorded on the
 * handle's stream around the launches (valid after finish/run). */
float nl_stack_last_kernel_ms(nl_stack_t *h);
/* Same, for the dominant kernel of the pass alone (the one named by
 * nl_stack_last_kernel_name); the difference is the hand-over passes. */
float nl_stack_last_dominant_kernel_ms(nl_stack_t *h);
/* GPU times of the pass enqueued `back` passes ago (0 = the last one): the handle keeps the
 * HIP events of its last 64 passes, so a caller may queue passes back to back without a host
 * sync and read every pass's kernel time afterwards.  Either output may be NULL. */
int nl_stack_pass_times(nl_stack_t *h, int back, float *pass_ms, float *dominant_ms);
/* The handle's hipStream_t (passes are enqueued on it) and the device address of the
 * {clip_low, clip_high} totals of the last pass (2 x uint64, valid once the pass has run on that
 * stream): a multi-process caller reduces them across ranks ON THE DEVICE -- e.g. RCCL
 * ncclAllReduce on this stream -- instead of a host round trip per pass (stack.go:193-198). */
void *nl_stack_stream(nl_stack_t *h);
void *nl_stack_counters_device_ptr(nl_stack_t *h);
/* Enqueues, behind the last pass on the handle's stream, a copy of those 16 bytes into a
 * caller-owned device buffer (zeros for modes without counters). */
int nl_stack_copy_counters_async(nl_stack_t *h, void *device_dst);
/* The passes enqueued from now on leave their {clip_low, clip_high} (two int64; then two more 64-bit words of
 * bookkeeping) in `device_buf` -- 32 bytes of device memory of the caller, on the handle's device -- instead of
 * the handle's own buffer; NULL goes back to the own buffer.  For a per-process launcher that reduces the counters
 * of every pass over the ranks on the device (RCCL, stack.go:193-198 is a mutex-protected sum over goroutines): with a
 * small ring of buffers -- pass i into buffer i mod 3, the all-reduce of pass i in place on the first 16 bytes while
 * pass i + 1 runs -- no copy kernel sits between a pass and its collective (bench.py; 11 us of a 0.27 ms pass on one of
 * eight row tiles of the headline stack).  nl_stack_finish reads the buffer of the LAST pass, i.e. whatever the
 * caller's collective has made of it by then.  A buffer must not be handed to a new pass before the collective of
 * the pass that wrote it last has finished. */
int nl_stack_set_counters_buffer(nl_stack_t *h, void *device_buf);
/* Makes `hip_stream` (a hipStream_t of the handle's device) wait for everything enqueued on the handle so far -- the passes
 * and what they leave in the counters buffer -- without the handle's stream waiting for anything: one event record on it, with
 * no system-scope fence (device work ordered against device work).  For the launcher above: the stream a collective is
 * issued from waits for pass i this way, and pass i + 1 follows pass i on the handle's stream undisturbed (bench.py; measured on
 * a 512-row share of the headline stack with a world-size-1 RCCL group: 0.2634 -> 0.2605 ms per step -- most of the 20 us a
 * step takes beyond its pass is the collective's own work on the device, not its bookkeeping).  No counterpart in the
 * reference. */
int nl_stack_order_stream_after(nl_stack_t *h, void *hip_stream);
/* on != 0: run every mode with the bit-exact kernels only (per-pixel replay
 * of the reference's permutation; slow, used for verification; 1 = one pixel
 * per lane with the column in LDS, 2 = one wavefront per pixel, 3 = one
 * wavefront per 64 consecutive pixels with their columns in LDS -- 2 and 3
 * exist for sigma and winsorized clipping, weighted or not; 4 (four pixels per
 * wavefront) was removed with the experiments build and fails with NL_ERR_INVALID_ARG; by default the weighted clip modes run 3
 * for shallow stacks, a decision pass + 2 for 33 ... 512 frames, 2 above).  Default 0:
 * sigma clipping uses the register-resident kernel, which keeps the clip
 * counters identical to the reference's and the output within summation-order
 * rounding, and hands undecidable pixels to the exact kernel. */
int nl_stack_set_exact(nl_stack_t *h, int on);
/* Developer switches of the sigma / winsorized fast path, for A/B timing inside one process (results are the
 * same either way): bit 0 = plain pass protocol (memset before, reduction kernel after every pass) instead of
 * the fused one, bit 1 = the exact replay of the dominant kernel's hand-overs runs in front of the generic pass
 * on the same stream instead of beside it (kernel traces then show each kernel's own duration), bit 2 = weighted
 * stacks replay every clipping round in full (no decision pass), bit 3 (8) = no effect (its replay was removed),
 * bit 4 (16) = weighted stacks skip the 64-pixels-per-wave tile replay (the next engine of the
 * table in DESIGN.md section 3 runs), bit 5 (32) = a pass records none of its three timing events (start, dominant
 * kernel start / end; nl_stack_pass_times then fails with NL_ERR_INVALID_ARG for that pass.  The event at the END of a
 * pass stays: asynchronous uploads order themselves behind it.  tools/wall_probe.py measures what the events cost),
 * bit 6 (64) = no effect (chunked passes were removed),
 * bit 7 (128) = winsorized passes of 16 ... 128 frames without the winsorization cascade,
 * bit 9 (512) = the first pass on a handle takes no list-length hints from earlier handles of the same geometry.
 * bits 10 (1024) and 11 (2048) selected the split and the persistent LDS-column pass (measured slower), bit 12
 * (4096) the guarded linear fit: their code was removed with the experiments build.
 * bit 13 (8192) = generic pass and first replay of a short-listed sigma pass on two streams (the protocol of rounds 2 - 4)
 * instead of one launch (stack_tail_fused.hip; also NL_TAIL_FUSED=0), for A/B runs.
 * bit 14 (16384) = winsorization loops without the invariant-interval certificate.
 * Default 0.  Bits 10 and 11 (like nl_stack_set_exact(h, 4)) are rejected with NL_ERR_INVALID_ARG ("removed with the experiments
 * build") instead of running another kernel under their name.
 * No counterpart in the reference. */
int nl_stack_set_dev_flags(nl_stack_t *h, unsigned flags);
/* Pixels of the last pass that were re-done by the exact kernel. */
int64_t nl_stack_last_fallback_pixels(nl_stack_t *h);
/* Pixels of the last pass that the dominant kernel handed to the generic pass (all positions
 * masked by rank: pixels that miss many samples or clip more than the clip zones hold). */
int64_t nl_stack_last_generic_pixels(nl_stack_t *h);
/* How the last pass was enqueued (diagnostics; the results do not depend on it): bit 0 = fused protocol (no memset in front, no
 * reduction kernel behind: sigma / winsorized passes once a handle knows its list lengths), bit 1 = generic pass and first
 * replay as one launch (plain sigma, 65 ... 128 frames, short exact lists; stack_tail_fused.hip).  No counterpart in the
 * reference. */
int nl_stack_last_pass_protocol(nl_stack_t *h);
/* Linear-fit cascade of the last pass (stack_linfit.hip; StackLinearFit stack.go:834-918 has no
 * counterpart, diagnostics only): counts[s] = pixels stage s handed to stage s+1 (4 stages; entries 4 ... 7 are zero).  Writes min(n, 8) values -- pass a buffer
 * of 8 -- and returns how many, 0 when the last pass ran no cascade. */
int nl_stack_linfit_stage_counts(nl_stack_t *h, unsigned *counts, int n);
/* Name of the dominant kernel launched by the last pass (for profiles). */
const char *nl_stack_last_kernel_name(nl_stack_t *h);

/* ---- goal-seek (spec: internal/ops/stack/stackfindsigma.go:27-170, FindSigmasAndStack) ----
 * Sigma / winsorized sigma (:48-98): bisection on sigma_low / sigma_high in [1,11] until
 * the clipped percentages match the targets to 0.01 % or 21 passes were made.
 * Linear fit (:101-170): Newton's method from (6, 6) with probe passes at +0.005, the
 * reference's quirks included (both high deltas are taken against the LOW target; the
 * step counter advances by three per iteration).  Other modes "do not support sigmas":
 * one pass with 0, 0; the returned sigmas are 0 (:42-46).  After each
 * pass the tile's {clip_low, clip_high} are handed to `reduce` (may be NULL
 * for a single tile) which must replace them with the totals over all tiles
 * -- e.g. an RCCL all-reduce -- so every rank takes the same branch.
 * The percentages are taken of width*height*n_frames (the WHOLE image) when a
 * reducer is given, of this handle's tile (rows*width*n_frames) when it is NULL. */
typedef int (*nl_reduce_fn)(int64_t *counters2, void *user);
int nl_stack_find_sigmas(nl_stack_t *h, int mode, float ref_loc,
                         float clip_perc_low, float clip_perc_high,
                         nl_reduce_fn reduce, void *user,
                         float *out_host, int64_t *clip_low, int64_t *clip_high,
                         float *sigma_low, float *sigma_high, int *passes);

/* ---- one stack over several GPUs from ONE process (stack.go:142-152, 193-198) ----
 * The reference's Apply splits the pixel range over goroutines and sums the two clip
 * counters over them; nl_group_* is that split over the GPUs of the node for a
 * single-process host (the Go CLI behind cgo, the C++ operator mirror): tile t owns the
 * rows nl_group_tile_rows(height, n_tiles, t) of all frames on devices[t] (devices ==
 * NULL: device t modulo the device count; n_tiles <= 0: one tile per device).  All
 * tiles' passes are enqueued before any is awaited; result tiles land in disjoint rows
 * of out_host; the counters are summed on the host.  Same arguments, error codes and
 * messages as the nl_stack_* calls they fan out to. */
typedef struct nl_group nl_group_t;
void nl_group_tile_rows(int height, int n_tiles, int t, int *row0, int *rows);
nl_group_t *nl_group_create(int n_frames, int width, int height, int n_tiles, const int *devices);
void nl_group_destroy(nl_group_t *g);
int nl_group_size(nl_group_t *g);
nl_stack_t *nl_group_tile(nl_group_t *g, int t);            /* borrowed, owned by the group */
int nl_group_upload_frame(nl_group_t *g, int idx, const float *host_frame);   /* overlapped, pointer not retained */
/* The ingest fast paths on the group (rows F3 / F4: internal/fits/read.go:351-395, project.go:26-76), overlapped
 * like nl_group_upload_frame -- one host thread per tile stages its share, nothing is awaited on the devices.
 * raw_host: the big-endian payload of the WHOLE frame (every tile takes the byte range of its rows);
 * src_host: the whole unaligned source frame (every tile projects its own rows). */
int nl_group_upload_frame_fits(nl_group_t *g, int idx, const void *raw_host, int bitpix, float bscale, float bzero,
                               float multiplier, float offset);
int nl_group_upload_frame_projected(nl_group_t *g, int idx, const float *src_host, int src_w, int src_h,
                                    const float trans[6], float out_of_bounds, float multiplier, float offset);
int nl_group_fill_synthetic(nl_group_t *g, uint64_t seed);
int nl_group_set_active_frames(nl_group_t *g, int n);
int nl_group_set_weights(nl_group_t *g, const float *weights);
int nl_group_set_exact(nl_group_t *g, int on);
int nl_group_run(nl_group_t *g, int mode, float sigma_low, float sigma_high, float ref_loc,
                 float *out_host, int64_t *clip_low, int64_t *clip_high);
int nl_group_last_mode(nl_group_t *g);
int nl_group_find_sigmas(nl_group_t *g, int mode, float ref_loc, float clip_perc_low, float clip_perc_high,
                         float *out_host, int64_t *clip_low, int64_t *clip_high,
                         float *sigma_low, float *sigma_high, int *passes);
int nl_group_accumulate(nl_group_t *g, float weight, int first);
int nl_group_accumulate_finalize(nl_group_t *g, float weight_sum, float *out_host);

/* ---- per-pixel rejection maps of a pass, coverage map of a stack ----
 * nl_stack_run_maps, nl_stack_coverage, nl_stack_last_coverage_ms, nl_group_run_maps, nl_group_coverage: declared in
 * nlstack_maps.h, which is part of this interface. */
#include "nlstack_maps.h"

/* ---- the same maps from the default pass's engines (sigma / winsorized clipping, unweighted, up to 128 frames) ----
 * nl_stack_run_maps_fast, nl_group_run_maps_fast: declared in nlstack_fastmaps.h, which is part of this interface. */
#include "nlstack_fastmaps.h"

/* ---- the same maps from the engines that keep a pixel's column in registers: those of nlstack_fastmaps.h, and the linear
 * fit's kernels with their cascade (1 ... 512 frames, bit-exact) ----
 * nl_stack_run_maps_resident, nl_group_run_maps_resident: declared in nlstack_residentmaps.h, which is part of this
 * interface. */
#include "nlstack_residentmaps.h"

/* ---- the same maps from the LDS-column engines of deep sigma / winsorized stacks (129 ... 512 frames, unweighted), and
 * from the engines of nlstack_residentmaps.h for everything else ----
 * nl_stack_run_maps_deep, nl_group_run_maps_deep: declared in nlstack_deepmaps.h, which is part of this interface. */
#include "nlstack_deepmaps.h"

/* ---- the same maps from the MAD-sigma engines (1 ... 512 frames, unweighted), the median on its default kernels with
 * zero maps, and the engines of nlstack_deepmaps.h for everything else ----
 * nl_stack_run_maps_full, nl_group_run_maps_full: declared in nlstack_fullmaps.h, which is part of this interface. */
#include "nlstack_fullmaps.h"

/* ---- linear-fit rejection with a weighted mean of the survivors (an extension: the reference's fit takes no weights) ----
 * nl_stack_run_linfit_weighted, nl_stack_run_linfit_weighted_async, nl_group_run_linfit_weighted: declared in
 * nlstack_wlinfit.h, which is part of this interface. */
#include "nlstack_wlinfit.h"

/* ---- sigma / winsorized rejection with a weighted mean whose weights follow their frames (an extension: the reference's
 * weights follow Hoare's permutation) ----
 * nl_stack_run_clip_weighted, nl_stack_run_clip_weighted_async, nl_group_run_clip_weighted: declared in
 * nlstack_wclip.h, which is part of this interface. */
#include "nlstack_wclip.h"

/* ---- MAD-sigma rejection with a weighted mean whose weights follow their frames (an extension: the reference panics
 * on MAD sigma with weights, and nl_stack_run keeps failing with NL_ERR_WEIGHTED_MAD) ----
 * nl_stack_run_mad_weighted, nl_stack_run_mad_weighted_async, nl_group_run_mad_weighted: declared in nlstack_wmad.h,
 * which is part of this interface. */
#include "nlstack_wmad.h"

/* ---- the median and MAD sigma of 513 ... 2048 frames on register-resident engines (an extension of depth, not of
 * semantics: the results are those of nl_stack_run; everything else falls through to nl_stack_run's pass) ----
 * nl_stack_run_deepstack, nl_stack_run_deepstack_async, nl_group_run_deepstack: declared in nlstack_deepstack.h, which
 * is part of this interface. */
#include "nlstack_deepstack.h"
#include "nlstack_deepstackmaps.h"
#include "nlstack_deepwmad.h"

/* ---- stack of stacks (StackIncremental / Finalize, stack.go:924-944) ----
 * acc += result_of_last_pass * weight (first != 0: acc = result*weight),
 * on the device; finalize multiplies by 1/weight_sum and downloads. */
int nl_stack_accumulate(nl_stack_t *h, float weight, int first);
int nl_stack_accumulate_finalize(nl_stack_t *h, float weight_sum, float *out_host);

/* ---- per-frame statistics on resident frames (internal/stats) ----
 * calcMinMeanMax + calcVariance (stats_amd64.s:28-143, stats.go:264-287):
 * min/max fp32, mean with fp64 accumulation, variance = sum((x-mean)^2)/n in
 * fp64.  NaN-free input is assumed, as in the reference. */
int nl_stack_frame_stats(nl_stack_t *h, int idx, float *mn, float *mean, float *mx,
                         double *variance);
/* EstimateNoise (stats/noise.go:32-55, noise_amd64.s:78-195).  Needs a
 * whole-image handle (row0=0, rows=height). */
int nl_stack_frame_noise(nl_stack_t *h, int idx, float *noise);
/* Noise of every frame -> inverse-noise weights -> nl_stack_set_weights
 * (stack.go:241-253).  noise_out: n_frames floats or NULL. */
int nl_stack_weights_from_noise(nl_stack_t *h, float *noise_out);

/* ---- Stats.Location() / Scale() of a resident frame (internal/stats/stats.go:225-244) ----
 * nl_stack_frame_location_scale, nl_location_scale, nl_locscale_seeds, nl_locscale_t and the NL_LSE_* estimators:
 * declared in nlstack_locscale.h, which is part of this interface. */
#include "nlstack_locscale.h"

/* ---- formats and steps either side of the stack (F3, F4) ----
 * A frame goes from its on-disk bytes to its slot of the stack buffer without
 * a CPU pass.  All of these are bit-exact restatements (elementwise fp32, the
 * reference's operation order).
 *
 * nl_stack_upload_frame_fits: internal/fits/read.go:172-445 (readUint8Data ..
 * readFloat64Data).  raw_host = the big-endian FITS payload bytes of exactly the
 * handle's tile (rows*width values of BITPIX 8/16/32/64/-32/-64; row-major, so
 * a row tile is a contiguous byte range of the file).  v = float32(val)*bscale
 * + bzero.  stats_out (3 floats or NULL) = min, max, mean of the decoded tile
 * (mean through an fp64 sum, read.go:210).  multiplier/offset: MatchHistogram
 * (internal/fits/pixelops.go:601-605) fused behind the decode; pass 1, 0 for
 * none (then nothing is applied). */
int nl_stack_upload_frame_fits(nl_stack_t *h, int idx, const void *raw_host, int bitpix,
                               float bscale, float bzero, float multiplier, float offset,
                               float *stats_out);
/* nl_stack_upload_frame_projected: Image.Project (internal/fits/project.go:26-76)
 * straight into the frame slot.  src_host = the WHOLE unaligned frame
 * (src_w x src_h fp32); trans = the forward Transform2D {A,B,C,D,E,F}
 * (internal/star/coord.go:52-59), inverted as coord.go:159-199 (singular ->
 * NL_ERR_INVALID_ARG, the reference returns an error too); bilinear taps with
 * the reference's fp32 expressions; destination pixels whose taps leave the
 * source get out_of_bounds (NaN in the pipeline = "no data" for the stack).
 * Only the handle's rows are produced.  multiplier/offset as above. */
/* Overlapped forms of the two calls above (no statistics): the bytes go through the pinned staging ring of
 * nl_stack_upload_frame_async, the DMA, the decode / projection kernel run on the copy stream, the call returns
 * without waiting for the device; the next nl_stack_run* waits for them on the device. */
int nl_stack_upload_frame_fits_async(nl_stack_t *h, int idx, const void *raw_host, int bitpix,
                                     float bscale, float bzero, float multiplier, float offset);
int nl_stack_upload_frame_projected_async(nl_stack_t *h, int idx, const float *src_host, int src_w, int src_h,
                                          const float trans[6], float out_of_bounds, float multiplier,
                                          float offset);
int nl_stack_upload_frame_projected(nl_stack_t *h, int idx, const float *src_host, int src_w,
                                    int src_h, const float trans[6], float out_of_bounds,
                                    float multiplier, float offset);
/* MatchHistogram on a resident frame: x = x*multiplier + offset (pixelops.go:601-605). */
int nl_stack_frame_affine(nl_stack_t *h, int idx, float multiplier, float offset);
/* The result tile of the last pass as FITS payload bytes: big-endian fp32, NaN
 * replaced by 0 (internal/fits/write.go:88, 182-200).  raw_host: rows*width*4 bytes. */
int nl_stack_download_result_fits(nl_stack_t *h, void *raw_host);
/* Stand-alone forms (host in, host out) of the decode and the projection. */
int nl_fits_decode(const void *raw_host, int bitpix, int64_t n, float bscale, float bzero,
                   float *out_host, float *stats_out, int device);
int nl_project_bilinear(const float *src_host, int src_w, int src_h, float *dst_host, int dst_w,
                        int dst_h, const float trans[6], float out_of_bounds, int device);

/* ---- 3x3 spatial median filter (internal/median/median3x3.go:26-110) ----
 * host in/out, width*height floats each; border rows/columns copied. */
int nl_median_filter_3x3(const float *in_host, float *out_host, int width, int height, int device);
/* ---- MedianFilter = GatherAndMedian over every pixel (internal/median/gather.go:26-38,
 * internal/ops/pre/badpixels.go:54-77, MedianFloat32 median3x3.go:115-119) ----
 * out[i] = median of in[i + mask[j]] over the offsets that fall inside [0, n); mask as
 * star.CreateMask builds it (findstars.go:187-200), at most 32 offsets.  Even counts
 * average the two middle values (qsort.go:68-82).  Where the whole neighbourhood exists
 * this equals the reference; at the data's edges the reference's value depends on the
 * leftovers of earlier calls in its scratch buffer, here it is the median of what exists. */
int nl_median_filter_mask(const float *in_host, float *out_host, int64_t n, const int32_t *mask,
                          int mask_len, int device);

/* ---- OpCalibrate and OpBadPixel, mono (internal/ops/pre/preprocess.go:68-195) ----
 * The per-frame steps of the reference's `stack` command in front of debayering and star detection
 * (cmd/nightlight/main.go:285-293).  Bit-exact: Subtract c = a - b (badpixels.go:107-111), Divide
 * c = b <= 0 ? a : (a*bMax)/b in fp32 (badpixels.go:114-123); bad pixels as BadPixelMap
 * (badpixels.go:32-51) finds them and MedianFilterSparse (badpixels.go:81-88) replaces them, in index
 * order and in place.  No CPU path: without a device every entry fails with NL_ERR_NO_DEVICE.
 *
 * nl_calib_create: OpCalibrate's masters resident on one device (dark / flat: width*height fp32 of
 * their own shape, either may be NULL but not both); the flat's Stats.Max() (stats.go:112-121) is
 * taken here over the whole flat.  Dark and flat of different shapes: NULL, nl_last_error() =
 * "dark dimensions [w h] differ from flat dimensions [w h]" (preprocess.go:144-147).  Read-only
 * afterwards: any number of threads may share one.  NULL on failure (message in nl_last_error()). */
typedef struct nl_calib nl_calib_t;
nl_calib_t *nl_calib_create(int device, const float *dark_host, int dark_width, int dark_height,
                            const float *flat_host, int flat_width, int flat_height);
void nl_calib_destroy(nl_calib_t *c);
int nl_calib_flat_max(const nl_calib_t *c, float *out);
/* OpCalibrate.Apply (preprocess.go:68-99) then OpBadPixel.Apply, mono branch (preprocess.go:180-195),
 * on one host frame of width x height, one device round trip.  c may be NULL (no masters).  A light
 * whose shape differs from the masters' fails with "<frame_id>: Light dimensions [w h] differ from
 * dark dimensions [w h]" (or "flat"), unless the pixel counts are equal: then the masters apply 1-D
 * (the reference's Seestar case, where it prints a warning the caller may print too).
 * sigma_low == 0 || sigma_high == 0: no bad-pixel step (removed 0, diff stats NaN).  A negative sigma
 * fails with NL_ERR_INVALID_ARG: the reference would flag the zero differences of the border -- the
 * one deviation.  removed_out: number of bad pixels (len(bpm)); diff_stats_out[2]: mean and
 * StdDev() of the local-median differences (Image.MedianDiffStats, which FindStars reads).
 * out_host may equal in_host.  frame_id only for the error strings.  Safe to call from several host
 * threads at once (each call has a stream and scratch of its own). */
int nl_preprocess_frame(const nl_calib_t *c, int frame_id, const float *in_host, float *out_host,
                        int width, int height, float sigma_low, float sigma_high,
                        int64_t *removed_out, float *diff_stats_out, int device);
/* The same steps on a resident frame slot.  Calibrate works on any row tile (the tile's 1-D range of
 * the masters; c on the handle's device; the slot index is the frame id of the error strings).  The
 * bad-pixel step needs a whole-image handle (3x3 stencil and a whole-frame std), like
 * nl_stack_frame_noise; a tile handle fails with NL_ERR_INVALID_ARG.  Thresholds are computed on the
 * device: the only host round trip is the read-back of removed_out / diff_stats_out at the end. */
int nl_stack_frame_calibrate(nl_stack_t *h, int idx, const nl_calib_t *c);
int nl_stack_frame_badpixel(nl_stack_t *h, int idx, float sigma_low, float sigma_high,
                            int64_t *removed_out, float *diff_stats_out);

/* ---- OpBadPixel, Bayer branch, and OpDebayer (internal/ops/pre/preprocess.go:180-251) ----
 * The colour-camera front of the `stack -debayer R|G|B -cfa ...` command: OpCalibrate, then
 * CosmeticCorrectionBayer (badpixels_bayer.go:26-351) on the chosen channel's pixels, then
 * DebayerBilinear (debayer.go:41-263) to one interpolated plane of (width - xOff) &~ 1 by
 * (height - yOff) &~ 1.  Bit-exact, the delta mean / std included.  CFA "RGGB" / "GRBG" / "GBRG" /
 * "BGGR" (or lower case), channel "R" / "G" / "B" (or lower case); the CFA is checked first.  Errors
 * are the reference's: "Unknown CFA value <cfa>", "Unknown debayering value <channel>".  A debayered
 * shape of 0 pixels fails with NL_ERR_INVALID_ARG (the reference divides by zero): the one deviation.
 *
 * nl_debayer_shape: the shape OpDebayer.Apply gives a width x height frame (preprocess.go:239-251,
 * debayer.go:26-66).  Host only, needs no device.  channel or cfa "" (or NULL): no debayer, the shape
 * is unchanged. */
int nl_debayer_shape(int width, int height, const char *channel, const char *cfa, int *out_width,
                     int *out_height);
/* OpCalibrate.Apply, OpBadPixel.Apply, OpDebayer.Apply (preprocess.go:68-99, 180-251) on one host
 * frame, one device round trip.  out_host holds nl_debayer_shape(width, height, channel, cfa) pixels;
 * *out_width / *out_height receive that shape.  Every branch of the operators applies:
 * sigma_low == 0 || sigma_high == 0: no bad-pixel step; channel "": the mono branch, and the result is
 * exactly nl_preprocess_frame's (its negative-sigma rejection included); channel set: the Bayer branch
 * (a negative sigma is well defined there and accepted), which needs a valid CFA even when OpDebayer
 * would not run; cfa "": no debayer.  removed_out: numRemoved (or the mono bad-pixel count);
 * stats_out[2]: mean and std of data - median over the channel (the Bayer branch leaves the image's
 * MedianDiffStats unset), the mono MedianDiffStats on the mono branch, NaN when no step ran.
 * Calibration errors as nl_preprocess_frame.  Safe to call from several host threads sharing c. */
int nl_preprocess_frame_cfa(const nl_calib_t *c, int frame_id, const float *in_host, int width,
                            int height, const char *channel, const char *cfa, float sigma_low,
                            float sigma_high, float *out_host, int *out_width, int *out_height,
                            int64_t *removed_out, float *stats_out, int device);
/* The same into resident slot idx: the raw mosaic goes to per-handle scratch (allocated on first use,
 * freed by nl_stack_destroy), is calibrated (c may be NULL; the slot index is the frame id of the error
 * strings) and corrected there, and the debayered plane is written into the slot at the handle's frame
 * stride: it never crosses PCIe.  Needs a whole-image handle whose shape is nl_debayer_shape(raw_width,
 * raw_height, channel, cfa) and a non-empty channel and CFA; anything else fails with
 * NL_ERR_INVALID_ARG (mono frames take nl_stack_upload_tile + nl_stack_frame_calibrate +
 * nl_stack_frame_badpixel).  The only device-to-host copy is removed_out / stats_out at the end. */
int nl_stack_upload_frame_cfa(nl_stack_t *h, int idx, const float *raw_host, int raw_width,
                              int raw_height, const nl_calib_t *c, const char *channel,
                              const char *cfa, float sigma_low, float sigma_high,
                              int64_t *removed_out, float *stats_out);

/* ---- OpStarDetect: star.FindStars (internal/star/findstars.go:59-103) ----
 * Bit-exact: the star list, sumOfShifts and avgHFR are the reference's bits wherever the reference
 * returns.  nl_star_t is star.Star (findstars.go:30-37): same field order and size, so a cgo caller can
 * copy it straight into a []star.Star.
 *
 * location, scale: the caller's f.Stats.Location() / Scale(), as OpStarDetect.Apply passes them
 * (pre/preprocess.go:448); nl_stack_frame_location_scale estimates them on the resident frame.  diff_std: f.MedianDiffStats.StdDev()
 * (nl_stack_frame_badpixel's diff_stats_out[1]); NaN means MedianDiffStats == nil.  At most capacity
 * stars are written to stars_out; *n_stars always receives the full count.  sum_of_shifts, avg_hfr:
 * FindStars' other two results (avg_hfr is NaN when no star is left, 0/0 as there).  n_stars,
 * sum_of_shifts, avg_hfr may be NULL.  Without a device every entry fails with NL_ERR_NO_DEVICE.
 * Deviations, all NL_ERR_INVALID_ARG unless stated:
 *   1. diff_std NaN with bp_sigma > 0: the reference estimates the std from a random 1 % sample drawn with
 *      an unseeded generator (findstars.go:139-149).  Here every pixel whose whole 3x3 mask lies inside
 *      the data gives data[i] - MedianFloat32Slice9(gather), reduced by Stats.StdDev's arithmetic (fp64
 *      sums, float32 mean and std); the candidate loop starts from a zeroed buffer as with given stats.
 *   2. radius < 0 or radius > 1024 (radius 0 is well defined and finds no star).
 *   3. +-Inf anywhere in the frame.
 *   4. where the reference panics, with a message naming the site: a NaN Mass as the pivot of
 *      QPartitionStarsDesc (qsort.go:37-57), and a star whose bin lies outside filterOutOverlaps' grid
 *      (findstars.go:250-256: a NaN centroid after a NaN pixel in its window, or a centroid the 1-D wrap
 *      pulled past the last cell row). */
typedef struct nl_star {
    int32_t index;                 /* int32(x) + width*int32(y) */
    float value, x, y, mass, hfr;
} nl_star_t;
#ifdef __cplusplus
static_assert(sizeof(nl_star_t) == 24, "nl_star_t is star.Star: 24 bytes");
#else
_Static_assert(sizeof(nl_star_t) == 24, "nl_star_t is star.Star: 24 bytes");
#endif
/* One host frame of width x height, one device round trip for the frame plus three short ones for the
 * star lists.  Safe to call from several host threads at once (each call has a stream and scratch of its
 * own). */
int nl_find_stars(const float *data_host, int width, int height, float location, float scale,
                  float star_sig, float bp_sigma, float star_in_out, int radius, float diff_std,
                  nl_star_t *stars_out, int capacity, int *n_stars, float *sum_of_shifts,
                  float *avg_hfr, int device);
/* The same on resident slot idx, or on the last pass's result still on the device; both need a
 * whole-image handle (FindStars indexes the data 1-D), and the result form a handle that has run a
 * pass.  The frame never crosses PCIe. */
int nl_stack_frame_find_stars(nl_stack_t *h, int idx, float location, float scale, float star_sig,
                              float bp_sigma, float star_in_out, int radius, float diff_std,
                              nl_star_t *stars_out, int capacity, int *n_stars, float *sum_of_shifts,
                              float *avg_hfr);
int nl_stack_result_find_stars(nl_stack_t *h, float location, float scale, float star_sig,
                               float bp_sigma, float star_in_out, int radius, float diff_std,
                               nl_star_t *stars_out, int capacity, int *n_stars, float *sum_of_shifts,
                               float *avg_hfr);

/* ---- OpAlign's estimate: star.Aligner up to the minimiser (internal/star/align.go:58-206) ----
 * nl_aligner_create, nl_aligner_destroy, nl_aligner_info, nl_aligner_match, nl_aligner_match_stars and their types:
 * declared in nlstack_align.h, which is part of this interface. */
#include "nlstack_align.h"

/* ---- OpBackExtract: pre.NewBackground + Background.Subtract / Render ----
 * (internal/ops/pre/preprocess.go:372-398, internal/ops/pre/background.go:68-462)
 * Bit-exact wherever the reference returns: the smoothed grid (cells_out), the info fields, the
 * subtracted frame and the rendered background.  grid_size <= 0 is OpBackExtract's no-op: NL_OK, every
 * bit of the frame unchanged, *info zeroed.  stars / n_stars: exactly what nl_*find_stars returned
 * (f.Stars).  background_out (NULL or width*height floats, host): Render(), as the op.Save branch needs
 * it; the subtracted frame is the same either way.  cells_out: the first min(cells_x*cells_y,
 * cells_capacity) cells, row-major.  info: what Background.String() prints, plus the geometry; may be
 * NULL.  Without a device both entries fail with NL_ERR_NO_DEVICE.
 * Deviations, all NL_ERR_INVALID_ARG with a message naming the site:
 *   1. where the reference panics: a cell with no sample after star masking, or with no sample below
 *      the trimming bound (QSelectFloat32 on an empty slice); a cell index outside [0, cells) in
 *      Subtract / Render (every grid one cell wide or tall); a cell larger than FitCell's buffer; a NaN
 *      pivot in one of the literal selects the host runs for cells holding a NaN.
 *   2. cells_x or cells_y is 0 (the image is smaller than half a grid cell): the reference divides by 0.
 *   3. clip leaves cells that stay NaN on every pass of interpolate (e.g. clip >= cells): the reference
 *      loops forever.
 *   4. where a cell's median rank is tied between -0 and +0, the device may return the other zero;
 *      cells and pixels then differ only in the sign of a zero (integer camera data hold no -0). */
typedef struct nl_background {
    int32_t cells_x, cells_y, outlier_cells;
    float spacing_x, spacing_y, min, max;
} nl_background_t;
/* One host frame, in place (data_host in and out), on a handle of its own per call: safe to call from
 * several host threads at once, like nl_find_stars. */
int nl_back_extract(float *data_host, int width, int height, int grid_size, float hfr_factor,
                    float sigma, int clip, const nl_star_t *stars, int n_stars,
                    float *background_out, float *cells_out, int cells_capacity,
                    nl_background_t *info, int device);
/* The same on resident slot idx of a whole-image handle (row tiles: NL_ERR_INVALID_ARG), in place:
 * the frame never crosses PCIe, only the cell grid and the Subtract tables do. */
int nl_stack_frame_back_extract(nl_stack_t *h, int idx, int grid_size, float hfr_factor, float sigma,
                                int clip, const nl_star_t *stars, int n_stars,
                                float *background_out, float *cells_out, int cells_capacity,
                                nl_background_t *info);

/* ---- OpDebandHoriz / OpDebandVert (internal/ops/pre/banding.go:61-132, :197-270) ----
 * Bit-exact wherever the reference returns: the frame, threshold and the factors' range.  Per row (horiz)
 * or column (vert) the percentile-th percentile of the samples <= threshold (QSelectFloat32 with
 * k = int(float32(n) * percentile * 0.01), :82-93) is selected on the device; the windows over those
 * percentiles, fixWindowEdge (:134-162), the window medians and the factors median / percentile run on
 * the host literally; then every pixel is multiplied by its row's / column's factor on the device.
 * threshold is MaxFloat32 when sigma == 0, else location + sigma * scale with the caller's
 * f.Stats.Location() / Scale() (as for nl_find_stars; from nl_stack_frame_location_scale when the frame is resident).
 * info (may be NULL): what the reference's log line prints, "... threshold %.2f, factors in [%.3f, %.3f]".
 * The operators' own guards -- percentile <= 0 or >= 100, and for horiz window <= 0 (:62, :198) -- are
 * no-ops: NL_OK, every bit of the frame unchanged, info = {threshold, 1, 0}.  Without a device every
 * entry fails with NL_ERR_NO_DEVICE.
 * Deviations, all NL_ERR_INVALID_ARG with a message naming the site:
 *   1. where the reference panics: a row / column with no sample <= threshold (QSelectFloat32 on an empty
 *      slice; a NaN threshold, a line of NaN, or of +Inf with sigma == 0); window <= 0 in vert (make with a
 *      negative length, QSelectMedianFloat32 of no element); an out-of-bounds index in one of the literal
 *      selects over a window (a NaN among the interpolated edge values).
 *   2. where the selected rank is tied between -0 and +0, the device may return the other zero: the factor
 *      is then the other infinity. */
typedef struct nl_deband {
    float threshold, lowest, highest;
} nl_deband_t;
/* One host frame, in place (data_host in and out), on a handle of its own per call: safe to call from
 * several host threads at once, like nl_preprocess_frame. */
int nl_deband_horiz(float *data_host, int width, int height, float percentile, int window, float sigma,
                    float location, float scale, nl_deband_t *info, int device);
int nl_deband_vert(float *data_host, int width, int height, float percentile, int window, float sigma,
                   float location, float scale, nl_deband_t *info, int device);
/* The same on resident slot idx of a whole-image handle, in place (the window needs every row's
 * percentile: row tiles fail with NL_ERR_INVALID_ARG, like nl_stack_frame_badpixel).  The frame never
 * crosses PCIe, only the percentiles (down) and the factors (up) do. */
int nl_stack_frame_deband_horiz(nl_stack_t *h, int idx, float percentile, int window, float sigma,
                                float location, float scale, nl_deband_t *info);
int nl_stack_frame_deband_vert(nl_stack_t *h, int idx, float percentile, int window, float sigma,
                               float location, float scale, nl_deband_t *info);

/* ---- OpBin: fits.NewImageBinNxN (internal/ops/pre/preprocess.go:324-331, internal/fits/fits.go:163-195) ----
 * Bit-exact: every output pixel is the reference's fp32 sum over yoff then xoff, times
 * 1.0 / float32(n * n).  The output is width / n by height / n (the remainder columns and rows are
 * dropped); n <= 1 is OpBin's no-op.  (OpScaleOffset, which precedes OpBin in the reference's sequence,
 * is nl_stack_frame_affine.)
 * Deviation: a binned shape of 0 pixels (n > width or n > height) fails with NL_ERR_INVALID_ARG.
 *
 * nl_bin_shape: the shape OpBin gives a width x height frame.  Host only, needs no device. */
int nl_bin_shape(int width, int height, int n, int *out_width, int *out_height);
/* One host frame into out_host of nl_bin_shape pixels (n <= 1: a copy), on handles of its own per call:
 * safe to call from several host threads at once. */
int nl_bin_nxn(const float *in_host, int width, int height, int n, float *out_host, int device);
/* Resident slot src_idx of one whole-image handle binned into slot dst_idx of another on the same device,
 * whose shape is nl_bin_shape of the source's (n <= 1: a device copy); neither frame crosses PCIe.  The
 * destination's stream waits on the source's.  Intended use: a one-frame staging handle of the raw shape
 * (calibrate, bad pixels, deband) binned into the stack handle.  Row tiles, handles on different devices,
 * a shape mismatch and a destination whose frames are attached, not owned, fail with NL_ERR_INVALID_ARG. */
int nl_stack_frame_bin_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, int n);

/* ---- OpAlign's projection from a resident frame (internal/ops/post/postprocess.go:185) ----
 * OpAlign's f.Project (post/postprocess.go:185, fits/project.go:26-76) from a resident frame:
 * slot src_idx of the whole-image handle src, resampled through trans into slot dst_idx of dst
 * (any row tile: only dst's rows are produced).  out_of_bounds as OpAlign chooses it
 * (NaN / reference location / own location).  No multiplier/offset: MatchHistogram precedes
 * Align in the reference, so call nl_stack_frame_affine on the source slot first.
 * trans is the forward Transform2D, inverted as for nl_stack_upload_frame_projected (a singular one fails with
 * "Matrix has no inverse"); the result is bit-identical to that call's on the same source (another kernel, the same arithmetic).  Synchronous: on return
 * the source slot may be overwritten.  The source stays as it is.  NL_ERR_INVALID_ARG: a row-tile source, handles
 * on different devices (nl_stack_ form), the same slot of the same handle (a projection cannot run in place), a
 * destination whose frames are attached, not owned, a null trans, an index out of range.
 * The group form fans out over the tiles: a tile on the source's device projects straight from the source slot, a
 * tile on another device first receives the source rows it can tap by a peer-to-peer copy into its ingest buffer.
 * Nothing goes through host memory. */
int nl_stack_frame_project_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx,
                                const float trans[6], float out_of_bounds);
int nl_group_frame_project_from(nl_group_t *g, int idx, nl_stack_t *src, int src_idx,
                                const float trans[6], float out_of_bounds);
/* Developer query: of the workgroup tiles that nl_stack_frame_project_from(dst, ., src, src_idx, trans, .) launches, how
 * many stage their source box in LDS and how many take their taps from global memory.  Host
 * arithmetic only, the kernel's own.  Developer switches of nl_stack_set_dev_flags on dst, for A/B runs (the results
 * are the same either way): bit 15 (32768) = no tile stages, bit 16 (65536) = plain instead of nontemporal result
 * stores; they hold for the resident projections into dst.  No counterpart in the reference. */
int nl_stack_project_tile_paths(nl_stack_t *dst, nl_stack_t *src, int src_idx, const float trans[6],
                                int64_t *staged, int64_t *direct);

/* The same projection with a bicubic or Lanczos-3 resampling kernel (AN EXTENSION: the reference resamples
 * bilinearly): nl_stack_frame_resample_from, nl_group_frame_resample_from, nl_stack_resample_tile_paths and
 * nl_resample_lanczos3_table are declared in nlstack_resample.h, which is part of this interface. */
#include "nlstack_resample.h"

/* Drizzle integration of resident frames onto a finer output grid (AN EXTENSION: the reference has no drizzle):
 * nl_drizzle_geometry, nl_stack_frame_drizzle_from, nl_stack_drizzle_finalize, nl_stack_frame_reject_against and
 * nl_stack_drizzle_tile_paths are declared in nlstack_drizzle.h, which is part of this interface. */
#include "nlstack_drizzle.h"

/* CFA drizzle: a raw Bayer mosaic laid onto one colour plane with no debayer in front (AN EXTENSION):
 * nl_drizzle_cfa_transform, nl_stack_frame_drizzle_cfa_from, nl_stack_frame_reject_against_cfa and
 * nl_stack_frame_badpixel_cfa are declared in nlstack_cfadrizzle.h, which is part of this interface. */
#include "nlstack_cfadrizzle.h"

/* Square drizzle: the exact overlap of a rotated drop with an output pixel, mono and CFA (AN EXTENSION):
 * nl_drizzle_square_geometry, nl_stack_frame_drizzle_square_from, nl_stack_frame_drizzle_square_cfa_from and
 * nl_stack_drizzle_square_tile_paths are declared in nlstack_sqdrizzle.h, which is part of this interface. */
#include "nlstack_sqdrizzle.h"

/* ---- OpGaussianBlur / OpUnsharpMask / OpHSLUnsharpMask's UnsharpMask ----
 * (internal/ops/stretch/stretch.go:339-424, internal/ops/stretch/usm.go, internal/ops/hsl/hsl.go:538-551)
 * The two passes of GaussFilter2D (usm.go:118-122): Convolve1DX (usm.go:85-98) into a scratch frame of the
 * handle, Convolve1DY (usm.go:101-114) back, every output sum = 0, then sum = sum + data[reflect(. + i)] *
 * kernel[i + k] for i = -k .. k in fp32, one multiply and one add each; the unsharp mask adds
 * ApplyUnsharpMask (usm.go:134-149) to the second pass: d < abs_threshold copies d, else
 * r = d + (d - blurred) * gain, then r < min, then r > max, in that order (NaN falls through every test).
 * Bit-exact given the taps.  One reservation for the sigma forms: their taps go through the C library's
 * fp64 erf, which may differ from Go's math.Erf in the last place, so a tap may differ by one fp32 ulp from
 * the Go binary's; everything after the taps is bit-exact, and nl_convolve_separable has no reservation.
 * min, max and abs_threshold are the caller's scalars (OpUnsharpMask: f.Stats.Min(), f.Stats.Max(),
 * Location() + Scale() * Threshold; OpHSLUnsharpMask: the luminance plane's), as location / scale are for
 * nl_find_stars (nl_stack_frame_location_scale).  The operators' own guards -- sigma == 0 in the blur and unsharp-mask entries, gain == 0 in
 * the unsharp-mask entries (stretch.go:369, :414) -- are no-ops: NL_OK, every bit unchanged (the host
 * unsharp mask copies in to out).
 * Deviations, all NL_ERR_INVALID_ARG with a message naming the site:
 *   1. a sigma GaussianKernel1D cannot handle: NaN, negative or +Inf (its radius search never ends; the
 *      search here stops at a radius of 65536, more than any frame of < 2^31 pixels holds), one below the
 *      value at which the radius comes out -1 (about 0.215: make with a negative length panics), and
 *      sigma == 0 in nl_gaussian_kernel_1d itself.
 *   2. a radius above width or above height: one reflect (usm.go:25-33) leaves the range, the reference
 *      reads a neighbouring row or panics.
 *   3. an even or non-positive n_taps in nl_convolve_separable: the reference indexes past the kernel.
 *   4. a capacity below the tap count in nl_gaussian_kernel_1d (*n_taps_out still receives the count).
 *   5. a row-tile handle: the column pass needs every row (like nl_stack_frame_deband_horiz).
 *   6. the result forms on a handle that has not run a pass (like nl_stack_result_find_stars).
 *
 * GaussianKernel1D (usm.go:41-82): erf in fp64 on float64((x - mu) / (sqrt2 * sigma)), everything else in
 * fp32; the left half summed, the right half mirrored, every tap times 1.0 / sum.  Host only, needs no
 * device.  taps_out may be NULL with capacity 0 to ask for the count. */
int nl_gaussian_kernel_1d(float sigma, float *taps_out, int capacity, int *n_taps_out);
/* Convolve1DX then Convolve1DY (usm.go:85-114) of one host frame with the caller's n_taps taps, in place.
 * The host forms run on handles of their own per call: safe to call from several host threads at once. */
int nl_convolve_separable(float *data_host, int width, int height, const float *taps, int n_taps, int device);
/* GaussianBlur (usm.go:126-130) of one host frame, in place. */
int nl_gaussian_blur(float *data_host, int width, int height, float sigma, int device);
/* UnsharpMask (usm.go:153-159) of one host frame into out_host (which may be in_host). */
int nl_unsharp_mask(const float *in_host, float *out_host, int width, int height, float sigma, float gain,
                    float min, float max, float abs_threshold, int device);
/* The same on resident slot idx of a whole-image handle, in place: only the taps cross PCIe. */
int nl_stack_frame_gaussian_blur(nl_stack_t *h, int idx, float sigma);
int nl_stack_frame_unsharp_mask(nl_stack_t *h, int idx, float sigma, float gain, float min, float max,
                                float abs_threshold);
/* ... and on the last pass's result still on the device, in place (nl_stack_finish / a download after it
 * returns the filtered result). */
int nl_stack_result_gaussian_blur(nl_stack_t *h, float sigma);
int nl_stack_result_unsharp_mask(nl_stack_t *h, float sigma, float gain, float min, float max,
                                 float abs_threshold);
/* Developer query: whether the row pass and the column pass of a kernel of n_taps taps stage their source
 * tile in LDS (1) or take every tap from global memory (0).  Host arithmetic only,
 * the launcher's own; the results are the same either way.  No counterpart in the reference. */
int nl_blur_tap_paths(int n_taps, int *row_staged, int *col_staged);

/* ---- the tone curves of the stretch command, and OpSave's quantisation ----
 * (internal/ops/stretch/stretch.go:40-335 over internal/fits/pixelops.go; internal/fits/tiff16.go:108-135,
 * internal/fits/writejpg.go:106-131)
 * OpNormalizeRange, the two pixel passes OpStretchIterative chooses between, OpMidtones, OpGamma, OpGammaPP and
 * OpScaleBlack -- and the Apply...ToChannel calls of the OpHSL... operators on a luminance plane in a slot -- are one
 * per-pixel curve each, in place.  The caller passes what Go passes to the pixel function; the library derives the
 * loop constants as the reference does in front of its loop, in fp32 (and float64(1.0f / g) for the exponent):
 *   kind                     p[0], p[1], p[2]   per pixel d
 *   NL_TONE_SCALE_OFFSET     scale, offset      d * scale + offset                             (pixelops.go:123-128)
 *   NL_TONE_NORMALIZE        min, max           the same with scale = 1.0 / (max - min), offset = -min * scale
 *                                                                                              (:143-147)
 *   NL_TONE_GAMMA            g                  float32(pow(float64(d), gg)), gg = float64(1.0 / g)   (:151-157)
 *   NL_TONE_PARTIAL_GAMMA    from, to, g        where d > from && d < to: dd = (d - from) * rescale1,
 *                                               from + float32(pow(float64(dd), gg)) * rescale2 with rescale2 =
 *                                               to - from, rescale1 = 1.0 / rescale2; every other pixel, a NaN
 *                                               included, keeps its bits                       (:179-191)
 *   NL_TONE_MIDTONES         mid, black         value = d * (mid - 1) / ((2 * mid - 1) * d - mid); value < clipLow
 *                                               gives 0, else value > 1 gives 1; (value - clipLow) * scaler, with
 *                                               clipLow the same expression of black and scaler = 1 / (1 - clipLow);
 *                                               a NaN falls through both tests                 (:214-229)
 *   NL_TONE_SHIFT_BLACK      before, after      math.Max(0, (d - black) * scale) with black = (after - before) /
 *                                               (after - 1), scale = 1 / (1 - black): NaN for a NaN, +0 for -0 and
 *                                               for every negative product                     (:649-660)
 * fp32 without FMA, IEEE division; pow is the device's fp64 pow with C99's special cases, which Go documents
 * identically for everything these curves can reach (a negative base with a fractional exponent is NaN, +-0 to a
 * positive power 0 and to a negative one +Inf, an exponent of +Inf for g == 0).  Nothing the reference computes is
 * rejected.  One reservation: neither Go's math.Pow nor the device's pow is correctly rounded, so a pixel whose exact
 * power lies within a few fp64 ulps of the midpoint between two fp32 values may come out one fp32 ulp away from the Go
 * binary's; everything else is bit-exact.
 * Guards: g == 1 of NL_TONE_GAMMA (OpGamma.Apply, stretch.go:240) is a no-op that leaves every bit.  The g == 1 guard
 * of OpGammaPP (:279) and the guards of OpStretchIterative, OpMidtones and OpScaleBlack (:104, :196, :323) act on the
 * operator's fields, not on the pixel function's arguments: they stay with the caller.  Location() / Scale() are the
 * caller's scalars as everywhere else (nl_stack_frame_location_scale gives them without a download).
 * Statistics: every one of these curves ends in Stats.Clear(), and the next operator asks for Min() / Mean() / Max()
 * again.  mn, mean, mx are optional; when any is non-NULL the kernel also reduces what it writes, and the three
 * values are bit for bit what nl_stack_frame_stats would return on the slot immediately afterwards (a no-op fills
 * them too).  With all three NULL nothing is reduced.
 * Per-pixel steps: they run on row-tile handles as well and cover the tile only.
 * Errors, NL_ERR_INVALID_ARG with a message naming the site: an unknown kind, a NULL curve / frame / output, bits
 * other than 8 or 16, a result form on a handle that has not run a pass; and one deviation: a gamma of the export
 * that is NaN or <= 0 (the reference would convert an infinite value to an integer, which Go leaves to the
 * implementation).  Without a device every entry fails with NL_ERR_NO_DEVICE. */
#define NL_TONE_SCALE_OFFSET   0
#define NL_TONE_NORMALIZE      1
#define NL_TONE_GAMMA          2
#define NL_TONE_PARTIAL_GAMMA  3
#define NL_TONE_MIDTONES       4
#define NL_TONE_SHIFT_BLACK    5
typedef struct nl_tone {
    int32_t kind;   /* NL_TONE_* */
    float p[3];     /* the pixel function's arguments in the table's order; unused ones are ignored */
} nl_tone_t;
/* the curve on resident slot idx, in place */
int nl_stack_frame_tone(nl_stack_t *h, int idx, const nl_tone_t *tone, float *mn, float *mean, float *mx);
/* ... on the last pass's result still on the device, in place */
int nl_stack_result_tone(nl_stack_t *h, const nl_tone_t *tone, float *mn, float *mean, float *mx);
/* ... on n floats of host memory (n < 2^31), in place, on a handle of the call's own */
int nl_tone(float *data_host, int64_t n, const nl_tone_t *tone, float *mn, float *mean, float *mx, int device);
/* OpSave's pixel loop (WriteMonoTIFF16 / WriteMonoJPG): gray = (d - min) * scale with scale = 1 / (max - min) in
 * fp32; NaN or < 0 gives 0, > 1 gives 1; if gammaInv = float64(1.0 / gamma) != 1.0, float32(pow(float64(gray),
 * gammaInv)); then uint16(gray * 65535) (bits 16) or uint8(gray * 255) (bits 8) by truncation.  out_host receives
 * one count per pixel of the slot (of the tile, on a row-tile handle): bits 16 two bytes each, high byte first --
 * the layout of Go's image.Gray16.Pix, which tiff.Encode takes as it is -- bits 8 one byte each, image.Gray.Pix.
 * The frame stays as it is; 2 or 1 bytes per pixel cross PCIe instead of 4.  The pow reservation above applies:
 * such a pixel may be one count away. */
int nl_stack_frame_export_gray(nl_stack_t *h, int idx, float min, float max, float gamma, int bits, void *out_host);
int nl_stack_result_export_gray(nl_stack_t *h, float min, float max, float gamma, int bits, void *out_host);
int nl_export_gray(const float *data_host, int64_t n, float min, float max, float gamma, int bits, void *out_host,
                   int device);

/* ---- the rgb / lrgb command around its tone curves: combine, balance, chroma and hue steps, colour export ----
 * (internal/fits/rgb.go:43-281, internal/fits/pixelops.go:441-550 and :679-692, internal/fits/tiff16.go:45-91,
 * internal/fits/writejpg.go:43-89)
 * An RGB (or HCL / HSLuv) image is three slots of one whole-image handle, named by planes[3] in the reference's channel
 * order {0, 1, 2}: three distinct valid slot indices.  The entries take the planes as they are: the conversions between
 * colour spaces (RGBToHSLuv, HSLuvToRGB, MonoToHSLuvLum), SCNR and the target of OpHSLScaleBlack are go-colorful's
 * arithmetic, not the reference's own, and stay with the caller; Stats.Location() / Scale() are arguments as everywhere else
 * (one nl_stack_frame_location_scale per plane).
 * Everything here is bit-exact against the reference: fp32 without FMA, sums in its order, Go's Min / Max semantics (a
 * NaN stays NaN, -0 and every negative become +0); the two powers (NL_CHROMA_GAMMA, the export's gamma) carry the
 * reservation of the tone curves above (one fp32 ulp / one count at a rounding boundary).
 * Errors, NL_ERR_INVALID_ARG with a message naming the site: null pointers, bad or repeated plane indices, an unknown
 * kind, a whole-image step (darkest block, star intensity, balance) on a row-tile handle, and where the reference
 * would index out of range or convert a non-finite value: block < 1, border NaN or < 0 or so large that the first block
 * lies below 0, skip_bright / skip_dim that put the star range outside the list, a selected star whose HFR is NaN,
 * negative or gives a disc radius above 1024, an export gamma that is NaN or <= 0, bits other than 8 / 16.  Without a
 * device every entry but nl_rgb_normalization and nl_rgb_balance_coeffs fails with NL_ERR_NO_DEVICE. */
typedef struct nl_rgb { float r, g, b; } nl_rgb_t;               /* fits.RGB (rgb.go:28-32) */
/* getCommonNormalizationFactors (rgb.go:65-78): min and max over the channels' Stats.Min() / Max() by strict compares
 * from channel 0 on, mult = 1 / (max - min) in fp32.  Host only, needs no device. */
int nl_rgb_normalization(const float mins[3], const float maxs[3], float *min, float *mult);
/* The pixel loop of NewRGBFromChannels (rgb.go:55-60): dst slot dst_idx = (src slot src_idx - min) * mult, two fp32
 * roundings.  src_idx == -1 reads the last pass's result of src; dst == src with the same slot runs in place.  Same
 * device and same geometry (width, height, row tile); per-pixel, so row-tile handles are served. */
int nl_stack_frame_combine_from(nl_stack_t *dst, int dst_idx, nl_stack_t *src, int src_idx, float min, float mult);
/* ScaleOffsetClampRGB (pixelops.go:679-692): plane c = float32(math.Max(math.Min(1, float64(alpha[c] * d + beta[c])),
 * 0)), product and sum in fp32, the three planes in one launch.  stats_out is optional: {min, mean, max} of plane 0,
 * 1, 2 from the same pass, bit for bit what nl_stack_frame_stats returns on each slot afterwards.  Per-pixel. */
int nl_stack_rgb_scale_offset_clamp(nl_stack_t *h, const int planes[3], const float alpha[3], const float beta[3],
                                    float stats_out[9]);
/* findDarkestBlock (rgb.go:153-219): the mean colour of the block x block square with the lowest (r + g + b) / 3
 * inside the border; the first minimum in row-major order wins, a NaN never does, and with no block in range the
 * result is {MaxFloat32, MaxFloat32, MaxFloat32}.  The device computes every block's channel means (12 bytes per block
 * cross PCIe), the host scans them.  Developer switch of nl_stack_set_dev_flags: bit 17 (131072) = no strip is staged
 * in LDS (the results are the same). */
int nl_stack_rgb_darkest_block(nl_stack_t *h, const int planes[3], int block, float border, nl_rgb_t *out);
/* meanStarIntensity (rgb.go:223-281) over stars[sStart:sEnd] with sStart = int(float32(n) * skip_bright), sEnd = n -
 * int(float32(n) * skip_dim): per star the pixels within (0.75 HFR + 0.01) of its centre whose three channels lie
 * below clip, summed in the reference's order; the host folds the stars in order.  No star or an empty range gives
 * {0, 0, 0}; no pixel at all the reference's 0 * +Inf = NaN. */
int nl_stack_rgb_mean_star_intensity(nl_stack_t *h, const int planes[3], const nl_star_t *stars, int n_stars,
                                     float skip_bright, float skip_dim, nl_rgb_t clip, nl_rgb_t *out);
/* The scalar part of setBlackWhitePoints (rgb.go:125-145) in fp32, operation for operation.  Host only. */
int nl_rgb_balance_coeffs(nl_rgb_t cur_shadows, nl_rgb_t cur_highlights, nl_rgb_t target_shadows,
                          nl_rgb_t target_highlights, float alpha[3], float beta[3]);
/* what SetBlackWhitePoints logs: the coefficients of both passes, the darkest block and the mean star colour */
typedef struct nl_rgb_balance {
    float alpha1[3], beta1[3];     /* first pass: location -> shadows, location + 3 scale -> highlights */
    float alpha2[3], beta2[3];     /* second pass: darkest block -> shadows, mean star colour -> highlights */
    nl_rgb_t darkest, stars;
} nl_rgb_balance_t;
/* SetBlackWhitePoints (rgb.go:94-120), the whole of OpRGBBalance.Apply behind its zero-stars guard, which stays with
 * the caller: loc / scale are the channels' Stats.Location() / Scale() (nl_stack_frame_location_scale per plane); the first clamp pass also reduces the
 * statistics whose maxima times 0.9 clip the star pixels.  report may be NULL.  With the planes resident only the star
 * list, the block means and these scalars cross PCIe. */
int nl_stack_rgb_balance(nl_stack_t *h, const int planes[3], const nl_star_t *stars, int n_stars, int block,
                         float border, float skip_bright, float skip_dim, nl_rgb_t shadows, nl_rgb_t highlights,
                         const float loc[3], const float scale[3], nl_rgb_balance_t *report);
/* ... on 3 * width * height floats of host memory (plane after plane, fits.Image.Data), in place, on a handle of the
 * call's own */
int nl_rgb_balance(float *planar_host, int width, int height, const nl_star_t *stars, int n_stars, int block,
                   float border, float skip_bright, float skip_dim, nl_rgb_t shadows, nl_rgb_t highlights,
                   const float loc[3], const float scale[3], nl_rgb_balance_t *report, int device);
/* The chroma and hue steps of the OpHSL... operators (pixelops.go:441-550) on planes {h, c, l} (or {h, s, l}), one
 * elementwise in-place kernel each; only the plane the reference writes is written, a pixel it skips keeps its bits,
 * and a NaN in the deciding plane falls through the comparisons as in Go.  Per-pixel.
 *   kind                   p[0] ... p[3]               per pixel
 *   NL_CHROMA_GAMMA        gamma, threshold            l < threshold keeps c; else c = float32(pow(float64(c), gg)),
 *                                                      gg = float64(1.0 / gamma)                          (:448-455)
 *   NL_CHROMA_NEUTRALIZE   low, high                   as the reference computes it: it reads both bounds from .Low
 *                                                      (:473), so l < low zeroes c and every other pixel keeps its
 *                                                      bits; high is accepted and ignored                (:472-484)
 *   NL_CHROMA_FOR_HUES     from, to, factor            where (from <= to && h > from && h < to) || (from > to &&
 *                                                      (h > from || h < to)): c = float32(math.Max(0, math.Min(1,
 *                                                      float64(c * factor))))                            (:501-511)
 *   NL_ROTATE_HUES         from, to, offset, lthres    l < lthres keeps h; where the same hue test holds, h += offset
 *                                                                                                        (:530-543)
 * The operators' guards (Gamma == 1, Factor == 1, Offset == 0) act on their fields and stay with the caller. */
#define NL_CHROMA_GAMMA       0
#define NL_CHROMA_NEUTRALIZE  1
#define NL_CHROMA_FOR_HUES    2
#define NL_ROTATE_HUES        3
typedef struct nl_chroma {
    int32_t kind;   /* NL_CHROMA_* / NL_ROTATE_HUES */
    float p[4];     /* the pixel function's arguments in the table's order; unused ones are ignored */
} nl_chroma_t;
int nl_stack_rgb_chroma(nl_stack_t *h, const int planes[3], const nl_chroma_t *op);
/* The pixel loop of WriteTIFF16 (tiff16.go:50-87) / WriteJPG (writejpg.go:48-85), channel by channel as the gray export
 * above.  out_host receives per pixel R G B A: bits 16 four big-endian uint16 with A = 0xFFFF, 8 bytes -- the layout of
 * image.RGBA64.Pix -- bits 8 the bytes R G B 255 -- image.RGBA.Pix.  The planes stay as they are; 8 or 4 bytes per
 * pixel cross PCIe instead of 12.  Per-pixel. */
int nl_stack_rgb_export(nl_stack_t *h, const int planes[3], float min, float max, float gamma, int bits, void *out_host);
/* ... of 3 * n floats of host memory, plane after plane (n < 2^31), on a handle of the call's own */
int nl_export_rgb(const float *planar_host, int64_t n, float min, float max, float gamma, int bits, void *out_host,
                  int device);

/* ---- host-side operator mirror (nightlight_amd/host/, C++) ----
 * The reference's stack operator decoded from its JSON form and run through
 * MakePromises/Apply exactly as OpSequence would drive it
 * (internal/ops/operator.go:484-513, internal/ops/stack/stack.go:92-227), on
 * host frames (frames[i] == NULL is a frame skipped upstream, "(nil, nil)").
 * Returns 0 on success; on failure err_buf holds the reference's message.
 * log_buf receives what the operator wrote to Context.Log. */
int nl_host_op_stack_apply_json(const char *json, int n_frames, int width, int height,
                                const float *const *frames, const float *exposure,
                                const float *hfr, int device, int max_threads,
                                float *out, float *exposure_out,
                                char *log_buf, int log_cap, char *err_buf, int err_cap);
/* Devices every host-side operator of this process stacks on from now on: one row tile of
 * each stack per entry (nl_group_*); a device may repeat.  n <= 0: back to the `device`
 * argument of the calls below. */
int nl_host_set_devices(const int *devices, int n);
/* Unmarshal with defaults (stack.go:92-99), marshal back. */
const char *nl_host_op_stack_roundtrip_json(const char *json);
/* OpStackBatches (internal/ops/stack/stackbatches.go:46-217): partition the inputs
 * into batches that fit stack_memory_mb (Context.StackMemoryMB, operator.go:41),
 * stack every batch with the per-batch "stack" operator given as JSON, combine
 * the batch results with StackIncremental / StackIncrementalFinalize weighted by
 * the batch frame counts (stack.go:924-944) ON THE DEVICES (nl_group_accumulate).  Same log
 * lines and error strings; the permutation comes from a fixed-seed generator instead of Go's
 * math/rand and is sorted inside every batch as stackbatches.go:199-209 does.  perm_out
 * (n_frames ints or NULL): input index of every position, batches = consecutive runs. */
int nl_host_op_stack_batches_apply_json(const char *per_batch_json, int n_frames, int width,
                                        int height, const float *const *frames,
                                        const float *exposure, int device, int max_threads,
                                        int memory_mb, int stack_memory_mb, float *out,
                                        float *exposure_out, int *perm_out, char *log_buf, int log_cap,
                                        char *err_buf, int err_cap);

#ifdef __cplusplus
}
#endif
#endif
