// nlstack_pass.hip -- one stack pass of the C ABI, and what runs passes: goal-seek, the stack of stacks.
// run_async_impl sets a pass up, select_engine picks the engine that runs it; all pixel arithmetic runs in the kernels.
#include <cassert>
#include <mutex>

#include "goal_seek.hpp"
#include "launch_common.hpp"
#include "nlstack_internal.hpp"

using nl::MapsTier, nl::PassKind;

namespace {

constexpr int kListGrid = 2048;     // workgroups of the exact kernel in fallback-list mode
constexpr int kCoopGrid = 16384;    // workgroups (one wave each) of the wave-per-pixel exact replay
constexpr int kListLanes = 4;       // pixels per wave there: few pixels, keep divergence low
constexpr unsigned kFusedMaxList = 512;    // exact-list length up to which a pass runs the fused protocol
constexpr unsigned kTailFusedMaxList = 512;    // ... up to which generic pass and first replay share one launch (stack_tail_fused.hip)
// winsorization cascade, "clipping passes : winsorization rounds per pass : regions of the previous stage's list per
// workgroup" for every stage (the last one runs to the end): measured on 4096^2 -- up to 40 frames
// 16 / 24 frames 3.68 / 3.94 -> 2.97 / 3.07 ms, 41 ... 96 frames (64: 5.22 -> 4.59 ms); beyond that a continuing stage
// re-reads every cache line of the stack for an eighth of its pixels and the cascade loses (128 frames: 5.43 -> 5.83 ms)
constexpr const char *kWinsorPlanShallow = "1:6,1:12:4,0:0:4";   // (round 5, with the certificate: first stage 8 -> 6 rounds, three stages instead of four: 16 / 24 / 32 frames 2.34 / 2.78 / 2.97 -> 2.17 / 2.71 / 2.80 ms)
constexpr const char *kWinsorPlanDeep = "2:12,2:16:8,3:24:4,0:0:4";
constexpr int kWinsorCascadeMaxFrames = 96;

// Developer switches (nl_stack_set_dev_flags, include/nlstack.h): A/B measurements, the results are the same either way
constexpr unsigned kDevPlainProtocol = 1u;         // memset before, reduction kernel after every pass
constexpr unsigned kDevReplayInFront = 2u;         // first replay in front of the generic pass, on the same stream
constexpr unsigned kDevNoDecision = 4u;            // weighted stacks: no decision pass, no recorded rounds
constexpr unsigned kDevNoTile = 16u;               // weighted stacks skip the 64-pixels-per-wave tile replay
constexpr unsigned kDevUntimed = 32u;              // a pass records none of its timing events
constexpr unsigned kDevNoWinsorCascade = 128u;     // winsorized passes without the winsorization cascade
constexpr unsigned kDevNoSharedHints = 512u;       // no list-length hints from earlier handles of the same geometry
constexpr unsigned kDevRemovedPasses = 1024u | 2048u;     // split / persistent LDS-column pass: removed, rejected
constexpr unsigned kDevTwoStreamTail = 8192u;      // generic pass and first replay on two streams, not one launch
constexpr unsigned kDevNoCertificate = 16384u;     // winsorization loops without the invariant-interval certificate

// ---- list-length hints across handles ---------------------------------------------------------------------------------
// A pass sizes its replay grids and picks its protocol from the list lengths the last FINISHED pass on the handle
// reported.  A handle that lives for one Apply never has one: its pass ran with 16 384-workgroup replay grids and the
// plain protocol (headline stack: 2.04 instead of 1.73 ms).  The lengths are therefore also remembered per geometry --
// frames, tile pixels, mode, weighted -- in a small process-wide table: the next handle of that geometry starts from
// what the last one saw (stacks of one session resemble each other; a wrong hint costs time, never correctness:
// tests/test_gpu_pass_history.py runs hints that are wrong by orders of magnitude, both ways, against the oracle).
struct HintKey { int frames; int64_t npix; int mode; bool weighted; };
struct HintEntry { HintKey key; unsigned fb, gen; };
std::mutex g_hint_mu;
std::vector<HintEntry> g_hints;
constexpr size_t kHintEntries = 32;

void hints_store(const HintKey &k, unsigned fb, unsigned gen)
{
    std::lock_guard<std::mutex> lk(g_hint_mu);
    for (HintEntry &e : g_hints)
        if (e.key.frames == k.frames && e.key.npix == k.npix && e.key.mode == k.mode && e.key.weighted == k.weighted) {
            e.fb = fb; e.gen = gen;
            return;
        }
    if (g_hints.size() >= kHintEntries) g_hints.erase(g_hints.begin());
    g_hints.push_back({k, fb, gen});
}

bool hints_load(const HintKey &k, unsigned *fb, unsigned *gen)
{
    std::lock_guard<std::mutex> lk(g_hint_mu);
    for (const HintEntry &e : g_hints)
        if (e.key.frames == k.frames && e.key.npix == k.npix && e.key.mode == k.mode && e.key.weighted == k.weighted) {
            *fb = e.fb; *gen = e.gen;
            return true;
        }
    return false;
}

int next_pow2(int n)
{
    int p = 1;
    while (p < n) p <<= 1;
    return p;
}

}  // namespace

// Grid of a dense replay whose workgroups stride through the pixels (item = workgroup + i * grid): with a grid that
// is a multiple of the image width a workgroup would visit ONE image column throughout, and the few workgroups of the
// alignment borders -- NaN columns, every pixel a full replay -- would run three times as long as the rest with the
// device draining around them (measured: 5 400 of 8 192 waves in flight on average).  A multiple of 8 (the
// XCD-contiguous mapping wants whole sweeps) that shares no large factor with the width walks through the columns
// (at least 64 of them per workgroup).
static int dense_grid(int64_t items, int64_t max_grid, int width, int pixels_per_item)
{
    int64_t g = items < max_grid ? items : max_grid;
    if (g <= 8 || items <= g) return (int)g;                 // no second sweep: nothing to align with
    g &= ~(int64_t)7;
    auto gcd = [](int64_t x, int64_t y) { while (y) { const int64_t t = x % y; x = y; y = t; } return x; };
    const int64_t most = (int64_t)width / 64 > 8 * pixels_per_item ? (int64_t)width / 64 : 8 * pixels_per_item;       // >= 64 columns per workgroup
    for (int tries = 0; tries < 64 && g > 8 && gcd(g * pixels_per_item, (int64_t)width) > most; tries++) g -= 8;
    return (int)g;
}

int nl::auto_select_mode(int l)   // stack.go:45-55
{
    if (l >= 25) return NL_ST_LINEAR_FIT;
    if (l >= 15) return NL_ST_WINSOR_SIGMA;
    if (l >= 6) return NL_ST_SIGMA;
    return NL_ST_MEAN;
}

extern "C" {

// Linear-fit cascade buffers (stack_linfit.hip): two pixel lists and state arrays with lanes_per_pixel liveness masks
// (16 B) per pixel, allocated on first use.  nullptr (allocation failure): the kernels run as a single bit-exact stage.
static const nl::LinfitCascade *linfit_cascade(nl_stack_t *h, nl::LinfitCascade *out)
{
    if (!h->lf_tried) {
        // sized for the most lanes per pixel any active frame count of this handle can need
        h->lf_lanes = h->n_capacity <= 128 ? 1 : h->n_capacity <= 256 ? 2 : 4;
        h->lf_tried = true;
        if (dev_malloc(&h->d_lf_count, sizeof(unsigned) * nl::kLinfitCounters) != hipSuccess) {
            (void)hipGetLastError();
            h->d_lf_count = nullptr;
        }
        const size_t np = (size_t)h->npix;
        for (int i = 0; h->d_lf_count && i < 2; i++)
            if (cached_malloc((void **)&h->d_lf_list[i], sizeof(unsigned) * np, h->device) != hipSuccess ||
                cached_malloc((void **)&h->d_lf_state[i], sizeof(uint4) * np * (size_t)h->lf_lanes, h->device) != hipSuccess) {
                (void)hipGetLastError();
                if (h->d_lf_list[i]) { (void)hipFree(h->d_lf_list[i]); h->d_lf_list[i] = nullptr; }
                h->d_lf_state[i] = nullptr;
                (void)hipFree(h->d_lf_count);              // no cascade at all on this handle
                h->d_lf_count = nullptr;
            }
    }
    if (!h->d_lf_count) return nullptr;
    out->list[0] = h->d_lf_list[0]; out->list[1] = h->d_lf_list[1];
    out->state[0] = h->d_lf_state[0]; out->state[1] = h->d_lf_state[1];
    out->count = h->d_lf_count;
    out->capacity = (unsigned)h->npix;
    return out;
}

// Weighted sigma / winsorized stacks of 33 ... 512 frames run a decision pass in front of the bit-exact replay
// (33 ... 128 frames: stack_fast_decide.hip, 129 ... 512: the LDS-column kernel of the class, record-only), and
// unweighted winsorized passes above 128 frames put their decided rounds on record for the list replay: scratch for the
// thresholds, kBoundRounds * 8 + 1 bytes per pixel of the tile (1.1 GB for 4096^2), allocated by the first pass that
// wants it and held until the handle is destroyed; nl_stack_device_bytes() reports what a handle holds at any time.
// false: off (NL_WDECIDE=0, developer switch kDevNoDecision, allocation failed: those passes then run without it).
static bool ensure_bounds(nl_stack *h)
{
    static const bool on = [] { const char *e = getenv("NL_WDECIDE"); return !(e && e[0] == '0'); }();
    if (!on || (h->dev_flags & kDevNoDecision)) return false;
    if (h->d_bounds) return true;
    if (h->bounds_tried) return false;
    h->bounds_tried = true;
    // (through the cache: a handle per Apply of a weighted stack pays no hipMalloc / hipFree of 1.1 GB at 4096^2)
    if (cached_malloc((void **)&h->d_bounds, (size_t)nl::kBoundRounds * (size_t)h->npix * sizeof(float2), h->device) != hipSuccess ||
        cached_malloc((void **)&h->d_nrounds, (size_t)h->npix, h->device) != hipSuccess) {
        (void)hipGetLastError();
        if (h->d_bounds) { (void)hipFree(h->d_bounds); h->d_bounds = nullptr; }
        h->d_nrounds = nullptr;
        return false;
    }
    return true;
}

// The sigma / winsorized fast path from 17 frames on (a zonal kernel followed by a generic pass) runs the FUSED protocol
// (StackArgs::final): no memset in front of the pass -- the previous fused pass's dominant kernel zeroed this pass's
// scratch set, the two sets alternate -- and no reduction kernel behind it.  NL_FUSED=0 (developer switch) keeps
// memset + reduce_counters_kernel for A/B runs, and turns off the recorded rounds of winsorized passes above 128 frames.
static bool fused_protocol_on()
{
    static const bool on = [] { const char *e = getenv("NL_FUSED"); return !(e && e[0] == '0'); }();
    return on;
}

// ---- one stack pass: run_async_impl sets it up, select_engine picks the engine that runs it ----------------------------
//
// The ladder of the maps passes (nl::MapsTier).  A maps pass is a plain-protocol pass whose kernels
// also store each pixel's two clip counts in h->d_reject_map.  Its tier says on which engines it may run, and every tier
// includes the ones below it:
//   Column    (nl_stack_run_maps)           the one-pixel-per-lane column kernel, every mode but the mean;
//   Fast      (nl_stack_run_maps_fast)      and run_sigma_maps on the register-resident sigma / winsorized kernels, 2 ... 128 frames;
//   Resident  (nl_stack_run_maps_resident)  and run_listed's linear fit, on its own kernels and cascade;
//   Deep      (nl_stack_run_maps_deep)      and run_sigma_maps on the LDS-column sigma / winsorized kernels, 129 ... 512 frames;
//   Full      (nl_stack_run_maps_full)      and run_listed's MAD sigma on its own kernels, 1 ... 512 frames; the median on its
//                                           default kernels with the maps zeroed;
//   DeepStack (nl_stack_run_maps_deepstack) and, beyond 512 frames: run_deep_mad's MAD sigma and run_deep_median's median on 8 / 16
//                                           lanes per pixel (513 ... 2048 frames), run_dense_replay's sigma / winsorized clipping on
//                                           the wave-per-pixel replay over the whole tile.
// What no engine of its tier takes runs on the column kernel.  On every tier the pass takes part in none of what default
// passes remember from one another: it takes and leaves no list-length hints, never runs the fused protocol, and leaves the
// scratch sets as any other plain-protocol pass does; the linear fit drops the handle's weights as in every other
// unweighted entry (stack.go:158).  One more engine with per-pixel counts is one rung of maps_engine and nl::Form::Maps
// (stack_kernels.h) at its launch sites: the pass carries its form in PassSetup::form, and every launcher takes one.

// the engines, in the order select_engine tries them
enum class Engine {
    Mean,
    MedianRegisters,      // register-resident sorting network, up to 128 frames
    MedianMultiLane,      // 129 ... 512 frames, 2 or 4 lanes per pixel
    Listed,               // MAD sigma / linear fit, one- or multi-lane: dominant kernel + bit-exact replay of its list
    SigmaFast,            // sigma / winsorized: dominant kernel + generic pass, replays of the pixels both hand over
    SigmaMaps,            // the same kernels with the per-pixel counts, plain protocol (a maps pass from MapsTier::Fast on)
    WeightedTile,         // bit-exact replay, 64 consecutive pixels per wave with their columns in LDS
    DenseReplay,          // bit-exact wave-per-pixel replay over the whole tile (behind a decision pass where there is one)
    ExactColumns,         // bit-exact, one pixel per lane with its column in LDS: every mode, any depth
    // the extension passes (nl::PassKind), each on an engine of its own:
    LinfitWeighted,       // PassKind::WeightedLinfit
    ClipWeighted,         // PassKind::WeightedClip
    MadWeighted,          // PassKind::WeightedMad
    DeepMedian,           // PassKind::DeepStack, the median of 513 ... 2048 frames: 8 or 16 lanes per pixel
    DeepMad,              // PassKind::DeepStack, MAD sigma of 513 ... 2048 frames: the same, + bit-exact replay of its list
    DeepMadWeighted,      // PassKind::DeepWeightedMad: the same kernel record-only, the streaming kernel of the weighted clip pass
};

// what the prologue of the pass decided, for the engine
struct PassSetup {
    int mode;
    bool weighted;
    bool timed;               // the pass records its timing events (not with kDevUntimed)
    bool fused;               // fused protocol (fused_protocol_on; only the SigmaFast engine runs it)
    nl::StackArgs a;
    nl::Form form;            // of the pass's kernels: Maps behind a tier (a.reject_map is set), Follow for the weighted clip and
                              // MAD-sigma passes (a.weights is set), else Plain
    bool maps() const { return form == nl::Form::Maps; }
};

// the depth conditions of the 8- / 16-lane engines (PassKind::DeepStack, PassKind::DeepWeightedMad, MapsTier::DeepStack): not forced exact, a tile
// within its stride, and -- with `weighted` = false: the kernels are the unweighted ones -- deep_ml_supported
static bool deep_conditions(const nl_stack *h, int mode, bool weighted, const nl::StackArgs &a)
{
    return !h->force_exact && a.npix <= a.stride && nl::deep_ml_supported(mode, weighted, a.n_frames, a.stride);
}

// The ladder of a maps pass (a.reject_map set, never the mean): the first rung whose condition holds; what no engine of the
// tier takes runs on the one engine that carries the per-pixel counts out of every mode.  Default passes never come here.
static Engine maps_engine(const nl_stack *h, int mode, bool weighted, const nl::StackArgs &a, nl::MapsTier tier)
{
    const bool fast = !h->force_exact;
    const bool clip = mode == NL_ST_SIGMA || mode == NL_ST_WINSOR_SIGMA;
    const bool listed = fast && h->d_fb_list, both_lists = listed && h->d_gen_list;
    const int n = a.n_frames;
    if (tier >= nl::MapsTier::Fast && both_lists && clip && nl::fast_supported(mode, weighted, n, a.npix)) return Engine::SigmaMaps;
    if (tier >= nl::MapsTier::Resident && listed && mode == NL_ST_LINEAR_FIT &&
        (nl::linfit_fast_supported(mode, n, a.npix) || nl::linfit_ml_supported(mode, n, a.npix)))
        return Engine::Listed;
    if (tier >= nl::MapsTier::Deep && both_lists && clip && !weighted && nl::fast_ml_supported(mode, false, n, a.npix))
        return Engine::SigmaMaps;
    if (tier >= nl::MapsTier::Full && both_lists && mode == NL_ST_MAD_SIGMA && !weighted &&
        (nl::mad_fast_supported(mode, false, n, a.npix) || nl::fast_ml_supported(mode, false, n, a.npix)))
        return Engine::Listed;
    // (the median rejects nothing: its default kernels, the maps zeroed)
    if (tier >= nl::MapsTier::Full && fast && mode == NL_ST_MEDIAN && nl::fast_supported(mode, weighted, n, a.npix))
        return Engine::MedianRegisters;
    if (tier >= nl::MapsTier::Full && fast && mode == NL_ST_MEDIAN && nl::fast_ml_supported(mode, weighted, n, a.npix))
        return Engine::MedianMultiLane;
    // beyond 512 frames (include/nlstack_deepstackmaps.h): the engines of the deep pass, and the replay nl_stack_run runs there
    if (tier >= nl::MapsTier::DeepStack && !weighted && deep_conditions(h, mode, false, a)) {
        if (mode == NL_ST_MAD_SIGMA && h->d_fb_list) return Engine::DeepMad;
        if (mode == NL_ST_MEDIAN) return Engine::DeepMedian;
    }
    if (tier >= nl::MapsTier::DeepStack && fast && clip && !weighted && n > 512 && nl::coop_supported(mode, false, n))
        return Engine::DenseReplay;
    return Engine::ExactColumns;
}

// Pure: allocates nothing, enqueues nothing.  An extension pass has its engine; a maps pass climbs maps_engine's ladder
// (tier); for every other pass the first engine whose condition holds runs it.
static Engine select_engine(const nl_stack *h, nl::PassKind kind, int mode, bool weighted, const nl::StackArgs &a, nl::MapsTier tier)
{
    const bool fast = !h->force_exact;
    const int n = a.n_frames;
    if (kind == PassKind::DeepStack) {
        // The deep pass (include/nlstack_deepstack.h): its two engines where they hold -- the median, and MAD sigma on a handle
        // with an exact list -- and the ladder of the default pass, unchanged, for everything else: another mode or depth,
        // nl_stack_set_exact, a stride beyond the gather's 31-bit offsets.
        const bool deep = deep_conditions(h, mode, weighted, a);
        if (deep && mode == NL_ST_MEDIAN) return Engine::DeepMedian;
        if (deep && mode == NL_ST_MAD_SIGMA && h->d_fb_list) return Engine::DeepMad;
        kind = PassKind::Default;
    }
    if (kind == PassKind::DeepWeightedMad) {
        // The deep weighted MAD-sigma pass (include/nlstack_deepwmad.h): its engine where the depth conditions hold on a handle
        // with an exact list (the engine itself falls back to run_mad_weighted where the threshold record cannot be had),
        // and PassKind::WeightedMad's, unchanged, for everything else.
        // (the streaming kernel's exact list holds 32-bit pixel indices: launch_stack_clip_weighted's bound)
        if (deep_conditions(h, mode, false, a) && h->d_fb_list && a.npix < nl::kFastMaxPixels) return Engine::DeepMadWeighted;
        kind = PassKind::WeightedMad;
    }
    if (kind != PassKind::Default) {
        // Until these kinds had engines of their own here, the pass asked the ladder below, dispatched past its answer and
        // kept one thing of it: whether it was SigmaFast, which turns on hint loading, the fused protocol and its single
        // start event.  It never was.  All three kinds run with the handle's weights (the entries refuse a handle without
        // them), and with weights fast_supported and fast_ml_supported are 0 for sigma and winsorized sigma; for the
        // linear fit and MAD sigma, which are no clip modes, they are 0 anyway: the SigmaFast rung cannot hold.
        assert(weighted && !nl::fast_supported(mode, weighted, n, a.npix) && !nl::fast_ml_supported(mode, weighted, n, a.npix));
        return kind == PassKind::WeightedLinfit ? Engine::LinfitWeighted
               : kind == PassKind::WeightedClip ? Engine::ClipWeighted : Engine::MadWeighted;
    }
    if (mode == NL_ST_MEAN) return Engine::Mean;
    if (a.reject_map) return maps_engine(h, mode, weighted, a, tier);
    if (fast && mode == NL_ST_MEDIAN && nl::fast_supported(mode, weighted, n, a.npix)) return Engine::MedianRegisters;
    if (fast && mode == NL_ST_MEDIAN && nl::fast_ml_supported(mode, weighted, n, a.npix)) return Engine::MedianMultiLane;
    if (fast && h->d_fb_list &&
        (nl::mad_fast_supported(mode, weighted, n, a.npix) || (mode == NL_ST_MAD_SIGMA && nl::fast_ml_supported(mode, weighted, n, a.npix)) ||
         nl::linfit_ml_supported(mode, n, a.npix) || nl::linfit_fast_supported(mode, n, a.npix)))
        return Engine::Listed;
    if (fast && h->d_fb_list && (nl::fast_supported(mode, weighted, n, a.npix) || nl::fast_ml_supported(mode, weighted, n, a.npix)))
        return Engine::SigmaFast;
    // nl_stack_set_exact(h, 3) forces the tile replay, 2 the wave-per-pixel one (verification)
    if ((h->exact_flavour == 3 ||
         (fast && weighted && !(h->dev_flags & kDevNoTile) &&
          n <= (mode == NL_ST_WINSOR_SIGMA ? nl::kTileMaxFramesWinsor : nl::kTileMaxFramesSigma))) &&
        nl::tile_supported(mode, weighted, n))
        return Engine::WeightedTile;
    if ((h->exact_flavour == 2 || (fast && (weighted || n > 512))) && nl::coop_supported(mode, weighted, n))
        return Engine::DenseReplay;
    return Engine::ExactColumns;
}

// FastArgs of a dominant kernel that hands pixels to the exact replay (fb_*) and / or to the generic pass (gen_*)
static nl::FastArgs list_args(const nl_stack *h, bool exact_list, bool generic_list)
{
    nl::FastArgs f;
    memset(&f, 0, sizeof f);
    if (exact_list) {
        f.fb_list = h->d_fb_list;
        f.fb_count = h->d_fb_count;
        f.fb_capacity = (unsigned)h->npix;
    }
    if (generic_list) {
        f.gen_list = h->d_gen_list;                 // (nullptr for huge tiles: the median kernel then sorts in full everywhere)
        f.gen_count = h->d_fb_count + 1;
        f.gen_capacity = (unsigned)h->npix;
    }
    return f;
}

// how a pass of the plain protocol ends: the sharded clip counts (d_partial) -> the pass's totals (d_counters)
static hipError_t reduce_clip_slots(nl_stack *h)
{
    return nl::launch_reduce_counters(h->d_partial, nl::kClipSlots, h->d_counters, h->stream);
}

// The column kernel (stack_exact.hip) in the form of the pass -- Form::Follow: one column, planned with weighted = false --
// over the exact list (d_fb_list), kListLanes pixels per wave
static int replay_list(nl_stack *h, int mode, bool weighted, const nl::StackArgs &a, nl::Form form = nl::Form::Plain)
{
    int lanes = 0;
    size_t lds = 0;
    weighted = weighted && form != nl::Form::Follow;
    if (nl::exact_plan(mode, weighted, a.n_frames, a.n_pad, kListLanes, &lanes, &lds) != 0)
        return fail(NL_ERR_TOO_MANY_FRAMES, "%d frames do not fit the per-pixel LDS column (mode %d)", a.n_frames, mode);
    nl::StackArgs e = a;
    e.list = h->d_fb_list;
    e.list_count = h->d_fb_count;
    e.list_capacity = (unsigned)h->npix;
    const char *exact_name = "";
    NL_HIP(nl::launch_stack_exact(mode, weighted, e, lanes, kListGrid, lds, h->stream, &exact_name, form));
    return NL_OK;
}

// ... over the whole tile, as the dominant kernel of the pass: ev_dom1 is recorded behind it
static int columns_over_tile(nl_stack *h, int mode, bool weighted, nl::StackArgs a, nl::Form form = nl::Form::Plain)
{
    int lanes = 0;
    size_t lds = 0;
    weighted = weighted && form != nl::Form::Follow;
    if (nl::exact_plan(mode, weighted, a.n_frames, a.n_pad, 64, &lanes, &lds) != 0)
        return weighted && mode == NL_ST_LINEAR_FIT
                   ? fail(NL_ERR_TOO_MANY_FRAMES, "%d frames do not fit the per-pixel LDS columns of the weighted linear fit", a.n_frames)
                   : fail(NL_ERR_TOO_MANY_FRAMES, "%d frames do not fit the per-pixel LDS column (mode %d)", a.n_frames, mode);
    a.tiles = (a.npix + lanes - 1) / lanes;
    const int grid = (int)(a.tiles < (int64_t)h->max_grid ? a.tiles : (int64_t)h->max_grid);
    NL_HIP(nl::launch_stack_exact(mode, weighted, a, lanes, grid, lds, h->stream, &h->last_kernel, form));
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    return NL_OK;
}

// How the engines of the plain protocol end: the column kernel in the pass's form over the exact list (`listed`: a dominant
// kernel filled it) or over the whole tile, then the reduction of the sharded clip counts
static int end_on_columns(nl_stack *h, const PassSetup &p, const nl::StackArgs &a, bool listed, PassFacts *facts)
{
    const int rc = listed ? replay_list(h, p.mode, p.weighted, a, p.form) : columns_over_tile(h, p.mode, p.weighted, a, p.form);
    if (rc != NL_OK) return rc;
    NL_HIP(reduce_clip_slots(h));
    facts->has_counters = true;
    return NL_OK;
}

// a.bounds / a.nrounds point at the handle's threshold record; false: there is none (ensure_bounds), `a` stays as it is
static bool bounds_on_record(nl_stack *h, nl::StackArgs &a)
{
    if (!ensure_bounds(h)) return false;
    a.bounds = h->d_bounds;
    a.nrounds = h->d_nrounds;
    return true;
}

// Grids of the wave-per-pixel list replays: one wave per workgroup, grid-stride over a list whose length is only known on
// the device; launching 16 k workgroups for a few hundred pixels costs more than replaying them, so the length the last
// finished pass reported (nl_stack_finish) sizes the grid.  grid0: the dominant kernel's hand-overs, grid1: the generic
// pass's additions.
static void replay_grids(const nl_stack *h, int *grid0, int *grid1)
{
    *grid0 = kCoopGrid;
    *grid1 = kCoopGrid / 4;
    if (h->fb_hint) {
        const int want = next_pow2((int)(2u * (h->fb_hint - 1u) + 64u));
        *grid0 = want < 1024 ? 1024 : (want > kCoopGrid ? kCoopGrid : want);      // (a 256-workgroup floor measured the same)
        *grid1 = *grid0 / 4 < 512 ? 512 : *grid0 / 4;
    }
}

// The decision pass of a weighted sigma / winsorized stack in front of the whole-tile replay: it leaves the clip bounds of
// every round it can decide in a.bounds / a.nrounds.  33 ... 128 frames: the register-resident kernel; 129 ... 512: the
// LDS-column kernel of the frame-count class (Form::Record: no outputs, lists or counters; a pixel it would hand
// to the generic pass has no round on record).
static int decision_pass(nl_stack *h, const PassSetup &p, nl::StackArgs &a)
{
    if (!p.weighted || h->exact_flavour != 0 || p.mode == NL_ST_MEDIAN) return NL_OK;
    const char *ignored = "";
    if (nl::decide_supported(p.mode, a.n_frames, a.npix) && bounds_on_record(h, a))
        NL_HIP(nl::launch_stack_sigma_decide(a, h->stream, p.mode == NL_ST_WINSOR_SIGMA, &ignored));
    else if (nl::decide_ml_supported(p.mode, a.n_frames, a.npix) && bounds_on_record(h, a))
        NL_HIP(nl::launch_stack_sigma_mlz(a, nl::FastArgs{}, h->stream, &ignored, p.mode == NL_ST_WINSOR_SIGMA, nl::Form::Record));
    return NL_OK;
}

static int run_mean(nl_stack *h, const PassSetup &p, PassFacts *)
{
    // (a maps pass: the mean rejects nothing)
    if (p.maps()) NL_HIP(hipMemsetAsync(p.a.reject_map, 0, (size_t)p.a.npix * sizeof(unsigned), h->stream));
    NL_HIP(nl::launch_stack_mean(p.weighted, p.a, h->stream, &h->last_kernel));
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    return NL_OK;
}

// bit-exact: a register-resident sorting network (pixels with many missing samples are handed from the pruned-network
// kernel to the full-sort one) or, 129 ... 512 frames, 2 or 4 lanes per pixel
static int run_median(nl_stack *h, const PassSetup &p, bool multi_lane)
{
    // (a maps pass, MapsTier::Full: the median rejects nothing, as the mean)
    if (p.maps()) NL_HIP(hipMemsetAsync(p.a.reject_map, 0, (size_t)p.a.npix * sizeof(unsigned), h->stream));
    if (!multi_lane) {
        NL_HIP(nl::launch_stack_median_fast(p.a, list_args(h, false, true), h->stream, &h->last_kernel, h->ev_dom1));
    } else {
        NL_HIP(nl::launch_stack_median_ml(p.a, h->stream, &h->last_kernel));
        NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    }
    return NL_OK;
}

// MAD sigma / linear fit: register-resident, the exact kernel replays the pixels the dominant kernel lists.
// The linear fit of a maps pass (MapsTier::Resident and up) runs the same plain protocol on the handle's one stream, the same
// cascade, quotas and grids, with the MAPS instantiations of its kernels (stack_linfit_maps.hip) and of the column kernel:
//   1. the dominant kernel over the tile: every lane that does not hand its pixel to the exact list STORES the pixel's
//      word of the map, p_lo | p_hi << 16, whether the pixel is finished or goes on;
//   2. the continuation stages of the cascade: the lane that owns a listed pixel ADDS its stage's counts to that word
//      (load, add, store: a pixel is on a stage's list at most once, the stages are ordered on the stream);
//   3. the column kernel's MAPS instantiation over the exact list (the pixels with an infinite sample), which stores
//      theirs: no stage touched them;
//   4. the reduction of the sharded clip counters.
// Every word is first written by exactly one plain store of 1. or 3.; 2. only adds to words this pass wrote: no memset,
// no stale word of an earlier pass.  Both kernels are bit-exact, so the result is the bit-exact one as well.  The stage
// lengths stay in d_lf_count and the exact list's in the scratch set, with or without the map.
// MAD sigma of a maps pass (MapsTier::Full, include/nlstack_fullmaps.h), likewise plain and on the one stream: the MAPS
// instantiations of the dominant kernel (and, from 114 frames on, of the finisher of its hand-over list), where the lane
// that stores a pixel's result stores its word as well; then 3. and 4.  Both medians are order independent, so the
// counts need no guard: the only pixels left to 3. are those without a finite median.
static int run_listed(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    const nl::StackArgs &a = p.a;
    if (p.mode == NL_ST_MAD_SIGMA) {
        // counters exact (the bounds come from two medians); pixels with a non-finite median are replayed; 128 frames:
        // pixels with too few samples for the selection kernel go to the generic list
        const nl::FastArgs f = list_args(h, true, true);
        if (a.n_frames <= 128) NL_HIP(nl::launch_stack_mad_fast(a, f, h->stream, &h->last_kernel, p.form));
        else                   NL_HIP(nl::launch_stack_mad_ml(a, f, h->stream, &h->last_kernel, p.form));
        NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    } else {
        // bit-exact (sums run in sorted order; 129 ... 512 frames: 2 or 4 lanes per pixel, the sums chained through the
        // lanes); only pixels with an infinite sample are replayed
        const nl::FastArgs f = list_args(h, true, false);
        nl::LinfitCascade cascade;
        const nl::LinfitCascade *cas = linfit_cascade(h, &cascade);
        if (cas) NL_HIP(hipMemsetAsync(h->d_lf_count, 0, sizeof(unsigned) * nl::kLinfitCounters, h->stream));
        if (nl::linfit_ml_supported(p.mode, a.n_frames, a.npix))
            NL_HIP(nl::launch_stack_linfit_ml(a, f, cas, h->stream, &h->last_kernel, h->ev_dom1, p.form));
        else
            NL_HIP(nl::launch_stack_linfit_fast(a, f, cas, h->stream, &h->last_kernel, h->ev_dom1, p.form));
    }
    facts->used_fast = true;
    return end_on_columns(h, p, a, true, facts);
}

// A winsorization cascade plan (kWinsorPlan*, NL_WCAS), the dominant kernel first, the last stage runs to the end:
//   plan  := stage { "," stage }          at most nl::kCascadeStages stages
//   stage := passes ":" cap [ ":" group ]  clipping passes per wave, winsorization rounds per pass, regions of the previous
//                                          stage's list per workgroup (1 ... 16, default 4)
// Parsing stops at the first thing that is not a stage; the stages before it stand.
struct CascadePlan { int stages; int pass[nl::kCascadeStages], cap[nl::kCascadeStages], group[nl::kCascadeStages]; };
static CascadePlan parse_cascade_plan(const char *p)
{
    CascadePlan pl{};
    while (*p && pl.stages < nl::kCascadeStages) {
        char *end = nullptr;
        const long a1 = strtol(p, &end, 10);
        if (end == p || *end != ':') break;
        p = end + 1;
        const long a2 = strtol(p, &end, 10);
        if (end == p) break;
        long a3 = 4;
        if (*end == ':') { p = end + 1; a3 = strtol(p, &end, 10); if (end == p) break; }
        pl.pass[pl.stages] = (int)a1;
        pl.cap[pl.stages] = (int)a2;
        pl.group[pl.stages] = a3 < 1 ? 1 : (a3 > 16 ? 16 : (int)a3);
        pl.stages++;
        if (*end != ',') break;
        p = end + 1;
    }
    return pl;
}

// Winsorized fast passes: how the generic pass and the winsorization loops are budgeted.  true: the winsorization cascade runs
// (never without may_cascade: the fast maps pass, whose kernels have no continuation form).
static bool winsor_setup(nl_stack *h, int n_frames, nl::FastArgs &f, bool may_cascade = true)
{
    // winsorized generic passes and the stages of the cascade behind the dominant kernel: a wave runs for its slowest pixel,
    // and the few pixels whose winsorization loops take dozens of rounds are cheaper in the replay (NL_GEN_ROUND_CAP: rounds per clipping pass; 100 = the limit of every kernel)
    static const int cap_env = [] { const char *e = getenv("NL_GEN_ROUND_CAP"); return e ? atoi(e) : 0; }();
    // (measured per frame count on the bench stack; 12 / 13 frames -- the smallest stacks with a zonal kernel -- lose with 40)
    f.gen_round_cap = cap_env > 0 ? cap_env : (n_frames >= 48 ? 24 : (n_frames > 20 ? 32 : ((n_frames == 12 || n_frames == 13) ? 60 : 40)));
    // the invariant-interval certificate of the winsorization loops (stack_fast_sigma_impl.hpp): first trial after
    // cert_first rounds of a loop, then every cert_every; NL_WCERT="first,every" ("0" = off), developer switch kDevNoCertificate: off
    // (3, 3: measured best at 16 frames and within 2 % of the best at 24, profiles/r05_winsor_cert.txt)
    static const int cert_env[2] = {[] { const char *e = getenv("NL_WCERT"); return e ? atoi(e) : 3; }(),
                                    [] { const char *e = getenv("NL_WCERT"); const char *c = e ? strchr(e, ',') : nullptr; const int v = c ? atoi(c + 1) : 3; return v > 0 ? v : 1; }()};
    f.cert_first = (h->dev_flags & kDevNoCertificate) ? 0 : cert_env[0];
    f.cert_every = cert_env[1];
    // winsorized clipping of 16 ... 128 frames: the winsorization cascade (stack_fast_sigma_impl.hpp) -- the dominant
    // kernel and a second stage stop at a budget of rounds per wave and hand their unfinished pixels on, a third
    // stage finishes them.  Lists and states live in the buffers of the linear-fit cascade (same sizes, never in
    // use at the same time); their lengths in the scratch set.  NL_WCAS="b1,b2" sets the budgets, "0" turns it off;
    // developer switch kDevNoWinsorCascade: off (A/B inside one process)
    if (!may_cascade || n_frames > 128 || n_frames < 12 || (h->dev_flags & kDevNoWinsorCascade)) return false;
    static const CascadePlan env_plan = [] { const char *e = getenv("NL_WCAS"); return e ? parse_cascade_plan(e) : CascadePlan{}; }();
    static const bool env_off = [] { const char *e = getenv("NL_WCAS"); return e && e[0] == '0' && e[1] == 0; }();
    CascadePlan pl{};
    if (env_plan.stages >= 2) pl = env_plan;
    else if (n_frames <= kWinsorCascadeMaxFrames) pl = parse_cascade_plan(n_frames <= 40 ? kWinsorPlanShallow : kWinsorPlanDeep);
    nl::LinfitCascade cb;
    // (a list holds at most one entry per pixel of the tile, rounded up to whole workgroups: list and states of a
    // stage share one of the cascade's state arrays, 4 words per pixel; the region lengths take its pixel lists)
    if (env_off || pl.stages < 2 || h->npix < 65536 || !linfit_cascade(h, &cb)) return false;
    for (int i = 0; i < 2; i++) {
        unsigned *base = reinterpret_cast<unsigned *>(cb.state[i]);
        f.cas_list[i] = base;
        f.cas_state[i] = base + 2 * (size_t)h->npix;
        f.cas_count[i] = cb.list[i];
    }
    f.cas_stages = pl.stages;
    for (int k = 0; k < pl.stages; k++) { f.cas_pass[k] = pl.pass[k]; f.cas_cap[k] = pl.cap[k]; f.cas_group[k] = pl.group[k]; }
    return true;
}

// The first replay of a pass (list part 0) beside the generic part: on the side stream behind the fork event, with ev_join
// for the pass to wait on.  The fork event is ev_dom1, recorded behind the dominant kernel, unless the pass is untimed or
// cascade stages have filled the lists since: then ev_fork, recorded here.  kDevReplayInFront: on the pass's own stream.
static int fork_first_replay(nl_stack *h, int mode, const nl::StackArgs &first, int grid, bool cascade)
{
    const char *ignored = "";
    const bool own = (h->dev_flags & kDevUntimed) || cascade;
    if (own) NL_HIP(hipEventRecord(h->ev_fork, h->stream));
    const bool in_front = (h->dev_flags & kDevReplayInFront) != 0;
    const hipStream_t s = in_front ? h->stream : h->side_stream;
    if (!in_front) NL_HIP(hipStreamWaitEvent(h->side_stream, own ? h->ev_fork : h->ev_dom1, 0));
    NL_HIP(nl::launch_stack_sigma_coop(mode, first, grid, s, &ignored));
    NL_HIP(hipEventRecord(h->ev_join, s));
    return NL_OK;
}

// Sigma / winsorized clipping: a register-resident (up to 128 frames) or LDS-column (129 ... 512) dominant kernel, a generic
// pass over the pixels it hands over, and the bit-exact replay of the pixels either cannot decide: one wave per pixel where
// available.  The hand-overs of the dominant kernel are replayed on the side stream WHILE the generic pass runs (both only
// depend on the dominant kernel); what the generic pass adds to the list is replayed after it.
static int run_sigma_fast(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    const int mode = p.mode;
    const bool winsor = mode == NL_ST_WINSOR_SIGMA;
    nl::StackArgs a = p.a;
    // winsorized passes: the fast kernels put the thresholds of every round they decide on record, so that the
    // replay of a pixel that turns undecidable later skips the winsorization loops of the decided rounds
    // (from 129 frames on: C3 tile 5.28 -> 5.14 ms; at 128 frames most undecidable pixels are undecidable in
    // their first round and the stores cost the dominant kernel 0.6 %)
    if (winsor && a.n_frames > 128 && fused_protocol_on()) (void)bounds_on_record(h, a);
    // the wave-per-pixel replays of the exact list: the first of them to start stores 1 + the list's length in `snap`
    // (StackArgs::list_snap); part 0 is the list as the dominant part left it, part 1 the generic pass's additions
    unsigned *const snap = h->d_fb_count + 2;
    nl::FastArgs f = list_args(h, true, true);
    f.fb_snap = snap;
    f.gen_hint = h->gen_hint;
    const bool cascade = winsor && winsor_setup(h, a.n_frames, f);
    const bool coop = nl::coop_supported(mode, p.weighted, a.n_frames) != 0;
    nl::StackArgs first = a;
    first.list = h->d_fb_list;
    first.list_count = h->d_fb_count;
    first.list_capacity = (unsigned)h->npix;
    first.list_snap = snap;
    first.list_part = 0;
    nl::StackArgs second = first;
    second.list_part = 1;
    int grid0 = 0, grid1 = 0;
    replay_grids(h, &grid0, &grid1);
    // Short exact lists (plain sigma, 65 ... 128 frames, fused protocol): generic pass and first replay as the lower and the
    // upper workgroups of ONE launch (stack_tail_fused.hip) instead of two streams -- no fork, no join: the join alone costs
    // a 512-row tile 14 us of its 257.  Every workgroup of that launch claims the generic pass's 48 KiB of LDS (three per
    // CU), hence only while one wave per listed pixel fits the device at that rate.
    // NL_TAIL_FUSED=0 / developer switch kDevTwoStreamTail: the two-stream protocol (A/B).
    static const bool tail_fused_on = [] { const char *e = getenv("NL_TAIL_FUSED"); return !(e && e[0] == '0'); }();
    const bool tail_fused = tail_fused_on && !(h->dev_flags & (kDevTwoStreamTail | kDevReplayInFront)) && p.fused && coop && !cascade &&
                            nl::tail_fused_supported(mode, p.weighted, a.n_frames) != 0 && h->fb_hint != 0 &&
                            h->fb_hint - 1u <= kTailFusedMaxList;
    unsigned replay_blocks = h->fb_hint + 31u;        // one wave per listed pixel and some: the list's length is last pass's
    replay_blocks = replay_blocks < 64u ? 64u : replay_blocks > 768u ? 768u : replay_blocks;
    const hipEvent_t dominant_done = p.timed ? h->ev_dom1 : nullptr;
    const bool one_lane = a.n_frames <= 128;          // 129 ... 512 frames: 2 or 4 lanes per pixel, the LDS-column kernels
    if (one_lane) NL_HIP(nl::launch_stack_sigma_dominant(a, f, h->stream, &h->last_kernel, dominant_done, winsor));
    else          NL_HIP(nl::launch_stack_sigma_mlz(a, nl::whole_tile(f), h->stream, &h->last_kernel, winsor));
    if (!one_lane && dominant_done) NL_HIP(hipEventRecord(dominant_done, h->stream));
    if (coop && !tail_fused) {
        const int rc = fork_first_replay(h, mode, first, grid0, cascade);
        if (rc != NL_OK) return rc;
    }
    if (one_lane) NL_HIP(nl::launch_stack_sigma_generic(a, f, h->stream, winsor, nl::Form::Plain, tail_fused ? &first : nullptr, replay_blocks));
    else          NL_HIP(nl::launch_stack_sigma_mlg(a, nl::over_generic_list(nl::whole_tile(f)), nl::ml_generic_grid(a.n_frames, f.gen_hint), h->stream, winsor));
    if (coop) {
        const char *exact_name = "";
        NL_HIP(nl::launch_stack_sigma_coop(mode, second, grid1, h->stream, &exact_name));
        if (!tail_fused) NL_HIP(hipStreamWaitEvent(h->stream, h->ev_join, 0));
    } else {
        const int rc = replay_list(h, mode, p.weighted, a);
        if (rc != NL_OK) return rc;
    }
    if (!p.fused) {              // (a fused pass implies coop: every kernel of the pass is enqueued)
        // (the reduction zeroes the scratch set behind itself: no memset in front of the next pass)
        NL_HIP(nl::launch_reduce_counters(h->d_partial, nl::kClipSlots, h->d_counters, h->stream, h->d_fb_count, true));
        facts->zeroed_behind = true;
    }
    facts->has_counters = facts->used_fast = facts->lists = true;
    facts->fused = p.fused;
    facts->tail_fused = tail_fused;
    return NL_OK;
}

// Sigma / winsorized clipping of a maps pass (MapsTier::Fast: 2 ... 128 frames, include/nlstack_fastmaps.h; MapsTier::Deep:
// 129 ... 512 frames, include/nlstack_deepmaps.h), unweighted.  The kernels of run_sigma_fast in their MAPS instantiations
// (stack_fast_maps_impl.hpp; stack_fast_mlz_maps_*.hip, stack_fast_mlg.hip), each lane storing its pixel's two clip counts
// beside its result, in the PLAIN protocol on the handle's one stream -- no fused protocol or tail, no side stream, no
// cascade, no threshold record (a.bounds stays null), no hints read or left:
//   1. the dominant kernel over the tile -- up to 128 frames the register-resident one (below 16 frames: the generic kernel
//      over the whole tile, and 2. has nothing to do), beyond that the LDS-column kernel of the frame-count class;
//   2. the generic kernel over the generic list, on a fixed grid (beyond 128 frames: ml_generic_grid(n, 0));
//   3. the column kernel's MAPS instantiation over the exact list, once, behind both of them;
//   4. the reduction of the sharded clip counters.
// Every pixel's word of the map is written by exactly one of 1 - 3: by the lane that stores its result.  The two list
// lengths stay in the scratch set (as run_listed leaves them), where nl_stack_last_*_pixels read them: nothing sits
// behind the totals, so nl_stack_finish takes no hints from this pass.
static int run_sigma_maps(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    const bool winsor = p.mode == NL_ST_WINSOR_SIGMA;
    const nl::StackArgs &a = p.a;
    nl::FastArgs f = list_args(h, true, true);          // (no snapshot cell, no hint: fixed grids)
    if (winsor) (void)winsor_setup(h, a.n_frames, f, false);      // (the round cap of the generic pass, as run_sigma_fast sets it)
    const hipEvent_t dominant_done = p.timed ? h->ev_dom1 : nullptr;
    const bool one_lane = a.n_frames <= 128;          // 129 ... 512 frames: 2 or 4 lanes per pixel, the LDS-column kernels
    if (one_lane) NL_HIP(nl::launch_stack_sigma_dominant(a, f, h->stream, &h->last_kernel, dominant_done, winsor, p.form));
    else          NL_HIP(nl::launch_stack_sigma_mlz(a, nl::whole_tile(f), h->stream, &h->last_kernel, winsor, p.form));
    if (!one_lane && dominant_done) NL_HIP(hipEventRecord(dominant_done, h->stream));
    if (one_lane) NL_HIP(nl::launch_stack_sigma_generic(a, f, h->stream, winsor, p.form));
    else          NL_HIP(nl::launch_stack_sigma_mlg(a, nl::over_generic_list(nl::whole_tile(f)), nl::ml_generic_grid(a.n_frames, 0), h->stream, winsor, p.form));
    facts->used_fast = true;
    return end_on_columns(h, p, a, true, facts);        // (p.weighted is false: both rungs of this engine are unweighted kernels)
}

// Bit-exact replay over the whole tile, 64 consecutive pixels per wave with their columns in LDS, one pixel per lane:
// the default for weighted sigma / winsorized clipping (their result depends on the reference's permutation, so there
// is no register-resident shortcut) up to kTileMaxFrames* frames -- the LDS column limits it to one wave per SIMD at
// 128 frames, where the wave-per-pixel replay is faster (tools/replay_probe.py: 0.5 vs 1.5 ms per Mpixel at 32 frames,
// 7.7 vs 3.8 at 128)
static int run_weighted_tile(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    const int64_t tiles = (p.a.npix + 63) / 64;
    const int64_t g = tiles < (1 << 20) ? tiles : (1 << 20);
    NL_HIP(nl::launch_stack_sigma_tile(p.mode, p.a, (int)g, h->stream, &h->last_kernel));
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    NL_HIP(reduce_clip_slots(h));
    facts->has_counters = true;
    return NL_OK;
}

// The wave-per-pixel exact replay over the whole tile: the default for deeper weighted sigma / winsorized stacks (behind
// their decision pass) and beyond 512 frames
static int run_dense_replay(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    nl::StackArgs a = p.a;
    const int rc = decision_pass(h, p, a);
    if (rc != NL_OK) return rc;
    const int per_item = p.mode == NL_ST_MEDIAN ? 1 : nl::coop_group(a);
    // many short workgroups: neighbours that start together share the sectors they fetch, long-lived workgroups
    // drift apart (128 frames x 4096^2, weighted sigma: 34.7 ms with 8 192 workgroups, 31.6 with 16 384, 28.0 with
    // 65 536, 27.2 with 262 144; a 512-row tile of 64 frames: 2.50 / 2.26 / 2.07 / 2.08 ms)
    const int64_t items = a.npix / per_item;
    const int64_t most = 262144;
    const int g = dense_grid(items, most, h->width, per_item);
    // (a maps pass, MapsTier::DeepStack: unweighted sigma / winsorized clipping beyond 512 frames, the MAPS form of the replay)
    if (p.mode == NL_ST_MEDIAN) NL_HIP(nl::launch_stack_median_coop(a, (int)g, h->stream, &h->last_kernel));
    else                        NL_HIP(nl::launch_stack_sigma_coop(p.mode, a, (int)g, h->stream, &h->last_kernel, p.form));
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    NL_HIP(reduce_clip_slots(h));
    facts->has_counters = p.mode != NL_ST_MEDIAN;
    return NL_OK;
}

// one pixel per lane with its column in LDS: every mode at any depth (nl_stack_set_exact(h, 1), and what no other engine takes)
static int run_exact_columns(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    const int rc = end_on_columns(h, p, p.a, false, facts);
    facts->has_counters = p.mode != NL_ST_MEDIAN;           // (the median clips nothing)
    return rc;
}

// The weighted linear-fit pass (include/nlstack_wlinfit.h, an extension): up to 128 frames the register-resident kernel
// of stack_linfit_weighted.hip, which hands the pixels it cannot decide to the exact list, and the column kernel's
// <linfit,weighted> instantiation over that list; deeper stacks, handles without a list and nl_stack_set_exact: the
// column kernel over the whole tile.  Plain protocol throughout, as run_listed and run_exact_columns.
static int run_linfit_weighted(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    const nl::StackArgs &a = p.a;
    const bool listed = !h->force_exact && h->d_fb_list && nl::linfit_weighted_supported(a.n_frames, a.npix);
    if (listed) {
        NL_HIP(nl::launch_stack_linfit_weighted(a, list_args(h, true, false), h->stream, &h->last_kernel));
        NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
        facts->used_fast = true;
    }
    return end_on_columns(h, p, a, listed, facts);          // (p.weighted: this pass keeps the weights)
}

// The weighted clip pass whose weights follow their frames (include/nlstack_wclip.h, an extension): sigma / winsorized
// rejection, then the mean of the survivors, each with its own frame's weight.
//   1. the decision pass of the weighted stacks, unchanged (decision_pass: 33 ... 512 frames), or its shallow
//      instantiations (9 ... 32 frames, stack_fast_decide_shallow.hip): thresholds per pixel and round in h->d_bounds;
//   2. one streaming read of the frames under those thresholds (stack_clip_weighted.hip), which hands the pixels without
//      a complete record to the exact list;
//   3. the column kernel's <follow> instantiation over that list;
//   4. the reduction of the sharded clip counters.
// Up to 8 frames and beyond 512, after nl_stack_set_exact, on handles without a list and where the thresholds cannot be
// had (ensure_bounds): the column kernel over the whole tile.  Plain protocol throughout, as run_linfit_weighted.
static bool clip_weighted_decided(nl_stack *h, int mode, const nl::StackArgs &a)
{
    return !h->force_exact && h->d_fb_list && a.npix < nl::kFastMaxPixels &&
           (nl::decide_supported(mode, a.n_frames, a.npix) || nl::decide_ml_supported(mode, a.n_frames, a.npix) ||
            nl::decide_shallow_supported(mode, a.n_frames, a.npix));
}

static int run_clip_weighted(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    nl::StackArgs a = p.a;
    bool streamed = false;
    if (clip_weighted_decided(h, p.mode, a)) {
        const int rc = decision_pass(h, p, a);
        if (rc != NL_OK) return rc;
        if (!a.bounds && nl::decide_shallow_supported(p.mode, a.n_frames, a.npix) && bounds_on_record(h, a)) {
            const char *ignored = "";
            NL_HIP(nl::launch_stack_sigma_decide_shallow(a, h->stream, p.mode == NL_ST_WINSOR_SIGMA, &ignored));
        }
        streamed = a.bounds != nullptr;
    }
    if (streamed) {
        NL_HIP(nl::launch_stack_clip_weighted(a, list_args(h, true, false), h->stream, &h->last_kernel));
        NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
        facts->used_fast = true;
    }
    // (the <follow> column kernel computes its own bounds)
    a.bounds = nullptr;
    a.nrounds = nullptr;
    return end_on_columns(h, p, a, streamed, facts);
}

// The weighted MAD-sigma pass (include/nlstack_wmad.h, an extension): StackMADSigma's rejection on the values alone, then
// the mean of the survivors in frame order, each with its own frame's weight.  Every engine takes the bounds from two
// medians and accumulates through wclip_take under that one round, so all of them give the same bits.
//   1 ... 128 frames: the FOLLOW instantiations of the register-resident MAD kernels (launch_stack_mad_fast), whose second
//      read is in frame order; pixels without a finite median go to the exact list;
//   129 ... 512 frames: the record-only instantiation of the multi-lane MAD kernel leaves (lo, hi) per pixel in h->d_bounds,
//      and the streaming kernel of the weighted clip pass reads the frames once under them (one recorded round is a
//      complete record); it hands pixels without a finite median or without a sample to the exact list;
//   then the column kernel's <mad,follow> instantiation over that list, and the reduction of the sharded clip counters.
// Beyond 512 frames, after nl_stack_set_exact, on handles without a list and where the thresholds cannot be had
// (ensure_bounds): the column kernel over the whole tile.  Plain protocol throughout, as run_clip_weighted.
static int run_mad_weighted(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    nl::StackArgs a = p.a;
    const bool lists = !h->force_exact && h->d_fb_list != nullptr;
    bool listed = false;
    if (lists && nl::mad_fast_supported(p.mode, false, a.n_frames, a.npix)) {
        NL_HIP(nl::launch_stack_mad_fast(a, list_args(h, true, true), h->stream, &h->last_kernel, p.form));
        listed = true;
    } else if (lists && nl::fast_ml_supported(p.mode, false, a.n_frames, a.npix) && bounds_on_record(h, a)) {
        const char *ignored = "";
        NL_HIP(nl::launch_stack_mad_ml(a, nl::FastArgs{}, h->stream, &ignored, nl::Form::Record));
        NL_HIP(nl::launch_stack_clip_weighted(a, list_args(h, true, false), h->stream, &h->last_kernel, true));
        a.bounds = nullptr;
        a.nrounds = nullptr;
        listed = true;
    }
    if (listed) {
        NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
        facts->used_fast = true;
    }
    return end_on_columns(h, p, a, listed, facts);
}

// The deep pass (include/nlstack_deepstack.h, an extension of depth): the median and MAD sigma of 513 ... 2048 active frames
// on the kernels of the 129 ... 512-frame engines with 8 or 16 lanes per pixel (stack_fast_ml_deep.hip).  Both rest on order
// statistics alone: the median is bit-exact as Engine::MedianMultiLane's; MAD sigma runs as Engine::Listed's -- its kernel
// the dominant one of a plain-protocol pass, the pixels without a finite median on the exact list for the column kernel,
// then the reduction of the sharded clip counters.  No hints read or left, never the fused protocol.
// A maps pass (MapsTier::DeepStack, include/nlstack_deepstackmaps.h) runs both: the median behind a memset of the map, as
// run_median; MAD sigma in Form::Maps -- the lane that stores a pixel's result stores its word, and the column kernel's
// <mad,maps> replay writes the words of the exact list, as run_listed does for the Full tier.
static int run_deep_median(nl_stack *h, const PassSetup &p)
{
    if (p.maps()) NL_HIP(hipMemsetAsync(p.a.reject_map, 0, (size_t)p.a.npix * sizeof(unsigned), h->stream));
    NL_HIP(nl::launch_stack_median_ml_deep(p.a, h->stream, &h->last_kernel));
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    return NL_OK;
}

static int run_deep_mad(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    NL_HIP(nl::launch_stack_mad_ml_deep(p.a, list_args(h, true, false), h->stream, &h->last_kernel, p.form));
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    facts->used_fast = true;
    return end_on_columns(h, p, p.a, true, facts);
}

// The deep weighted MAD-sigma pass (include/nlstack_deepwmad.h): run_mad_weighted's 129 ... 512 branch with the 8- / 16-lane
// kernel -- record-only, it leaves (lo, hi) per pixel in h->d_bounds; the streaming kernel of the weighted clip pass reads
// the frames once under them and hands pixels without a finite median or without a sample to the exact list; then the
// column kernel's <mad,follow> instantiation over that list and the reduction.  Where the threshold record cannot be had
// (ensure_bounds) the pass is run_mad_weighted's.
static int run_deep_mad_weighted(nl_stack *h, const PassSetup &p, PassFacts *facts)
{
    nl::StackArgs a = p.a;
    if (!bounds_on_record(h, a)) return run_mad_weighted(h, p, facts);
    const char *ignored = "";
    NL_HIP(nl::launch_stack_mad_ml_deep(a, nl::FastArgs{}, h->stream, &ignored, nl::Form::Record));
    NL_HIP(nl::launch_stack_clip_weighted(a, list_args(h, true, false), h->stream, &h->last_kernel, true));
    a.bounds = nullptr;
    a.nrounds = nullptr;
    NL_HIP(hipEventRecord(h->ev_dom1, h->stream));
    facts->used_fast = true;
    return end_on_columns(h, p, a, true, facts);
}

// A pass that fails half-way (a launch or an event call after the first kernel) must not hand control back with work in
// flight on the handle's streams and its bookkeeping half-updated: whatever was enqueued is waited for, the scratch
// sets count as dirty, no list lengths or hints are taken from the broken pass.  The error of the failing call is kept.
static int settle_failed_pass(nl_stack_t *h, int rc)
{
    if (rc != NL_OK && h && h->stream) {
        const std::string keep = g_err;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        if (h->side_stream) (void)hipStreamSynchronize(h->side_stream);
        (void)hipGetLastError();
        h->last = PassFacts{};
        h->sets_clean = false;
        h->partial_clean = false;
        h->pending = false;
        g_err = keep;
    }
    return rc;
}

// req.tier: a maps pass, on the ladder described above the engines.  Like a maps pass, two more passes take part in nothing
// default passes remember from one another: the weighted linear-fit pass (PassKind::WeightedLinfit; `mode` is
// NL_ST_LINEAR_FIT), which keeps the weights the default linear fit drops and runs on run_linfit_weighted, and the weighted
// clip pass whose weights follow their frames (PassKind::WeightedClip; `mode` resolves to sigma or winsorized sigma), which
// runs on run_clip_weighted.  A third: the weighted MAD-sigma pass (PassKind::WeightedMad; `mode` is NL_ST_MAD_SIGMA), the one
// entry that takes MAD sigma with weights, on run_mad_weighted.
static int run_async_impl(nl_stack_t *h, const nl::PassRequest &req)
{
    NL_CHECK_HANDLE(h);
    const nl::MapsTier tier = req.tier;
    const float sigma_low = req.sigma_low, sigma_high = req.sigma_high, ref_loc = req.ref_loc;
    int mode = req.mode;
    const bool maps = tier != nl::MapsTier::None, wlinfit = req.kind == PassKind::WeightedLinfit, wclip = req.kind == PassKind::WeightedClip;
    const bool wmad = req.kind == PassKind::WeightedMad || req.kind == PassKind::DeepWeightedMad;
    // the extension passes take their weights from the handle: the entry's name, and where the unweighted pass is
    static const struct { PassKind kind; const char *entry, *unweighted; } kNeedWeights[] = {
        {PassKind::WeightedMad, "run_mad_weighted", "the unweighted pass is nl_stack_run with NL_ST_MAD_SIGMA"},
        {PassKind::DeepWeightedMad, "run_mad_weighted", "the unweighted pass is nl_stack_run with NL_ST_MAD_SIGMA"},
        {PassKind::WeightedClip, "run_clip_weighted", "the unweighted pass is nl_stack_run"},
        {PassKind::WeightedLinfit, "run_linfit_weighted", "the unweighted fit is nl_stack_run with NL_ST_LINEAR_FIT"},
    };
    for (const auto &e : kNeedWeights)
        if (req.kind == e.kind && !h->has_weights)
            return fail(NL_ERR_INVALID_ARG, "%s: the handle has no weights (nl_stack_set_weights); %s", e.entry, e.unweighted);
    if (mode < NL_ST_MEDIAN || mode > NL_ST_AUTO) return fail(NL_ERR_INVALID_MODE, "invalid stacking mode");
    if (mode == NL_ST_AUTO) mode = nl::auto_select_mode(h->n_frames);
    if (wclip && mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA)
        return fail(NL_ERR_INVALID_MODE, "run_clip_weighted: mode %d is neither NL_ST_SIGMA nor NL_ST_WINSOR_SIGMA", mode);
    bool weighted = h->has_weights;
    if (mode == NL_ST_MAD_SIGMA && weighted && !wmad)
        return fail(NL_ERR_WEIGHTED_MAD, "MADSigma stacking with weights is still unimplemented");
    if ((mode == NL_ST_LINEAR_FIT && !wlinfit) || mode == NL_ST_MEDIAN) weighted = false;  // stack.go:158,188-189
    if (maps) {
        // (a pixel's count is bounded by its samples: 16 bits hold it up to 65 535 frames)
        if (h->n_frames > 65535)
            return fail(NL_ERR_TOO_MANY_FRAMES, "run_maps: %d active frames, a uint16 map holds counts up to 65535", h->n_frames);
        if (!h->d_reject_map) NL_HIP(dev_malloc(&h->d_reject_map, (size_t)h->npix * sizeof(unsigned)));
    }

    if (h->uploads_pending) {
        // asynchronous uploads: the pass waits for the last DMA on the device
        const int last = (h->stage_next + kStageSlots - 1) % kStageSlots;
        NL_HIP(hipStreamWaitEvent(h->stream, h->stage_done[last], 0));
        h->uploads_pending = false;
    }

    nl::StackArgs a{};                  // (no list, no final counters, no bounds: the engines set what they use)
    a.frames = h->d_frames;
    a.stride = h->fstride;
    a.npix = h->npix;
    a.n_frames = h->n_frames;
    a.n_pad = next_pow2(h->n_frames);
    a.weights = weighted ? h->d_weights : nullptr;
    a.xstat = h->d_xstat;
    a.sig_lo = sigma_low; a.sig_hi = sigma_high; a.ref_loc = ref_loc;
    a.out = h->d_out;
    a.partial = h->d_partial;
    a.reject_map = maps ? h->d_reject_map : nullptr;

    {
        const int slot = (int)(h->pass_seq % kTimingRing);
        if (!h->ring_start[slot]) {
            NL_HIP(hipEventCreateWithFlags(&h->ring_start[slot], hipEventDefault | h->ev_rel));
            NL_HIP(hipEventCreateWithFlags(&h->ring_stop[slot], hipEventDefault | h->ev_rel));
            NL_HIP(hipEventCreateWithFlags(&h->ring_dom0[slot], hipEventDefault | h->ev_rel));
            NL_HIP(hipEventCreateWithFlags(&h->ring_dom1[slot], hipEventDefault | h->ev_rel));
        }
        h->ev_start = h->ring_start[slot]; h->ev_stop = h->ring_stop[slot];
        h->ev_dom0 = h->ring_dom0[slot]; h->ev_dom1 = h->ring_dom1[slot];
    }
    const bool timed = !(h->dev_flags & kDevUntimed);
    h->ring_timed[h->pass_seq % kTimingRing] = timed;
    if (timed) NL_HIP(hipEventRecord(h->ev_start, h->stream));
    const bool fused_on = fused_protocol_on();
    const Engine engine = select_engine(h, req.kind, mode, weighted, a, tier);
    const bool sigma_fast = engine == Engine::SigmaFast;
    // (only while the exact list is short -- the length the last finished pass reported: its replays add their
    // counts to ONE word, and thousands of workgroups doing that take longer than a reduction kernel)
    if (sigma_fast && h->fb_hint == 0 && !(h->dev_flags & kDevNoSharedHints)) {
        unsigned fb = 0, gen = 0;
        if (hints_load({a.n_frames, a.npix, mode, weighted}, &fb, &gen)) { h->fb_hint = fb; h->gen_hint = gen; }
    }
    h->last_weighted = weighted;
    const bool fused = fused_on && !(h->dev_flags & kDevPlainProtocol) && sigma_fast && a.n_frames > 8 && h->fb_hint != 0 &&
                       h->fb_hint - 1u < kFusedMaxList && nl::coop_supported(mode, weighted, a.n_frames) != 0;
    // Every event recorded on the pass's stream costs a few microseconds of it (three of them: 17 us of a 277 us pass on
    // a 512-row tile, tools/wall_probe.py): a fused pass that finds its scratch set clean has nothing between "start" and
    // "dominant kernel starts", and the event behind the dominant kernel is also the fork of the side stream.
    const bool one_start = timed && fused && h->sets_clean;
    h->ring_dom0_is_start[h->pass_seq % kTimingRing] = one_start;
    if (one_start) h->ev_dom0 = h->ev_start;
    if (fused) {
        if (h->sets_clean) h->cur_set ^= 1;
        else NL_HIP(hipMemsetAsync(h->d_sets, 0, 2 * kScratchBytes, h->stream));
        h->d_partial = h->d_sets + (size_t)h->cur_set * nl::kScratchWords;
        h->d_fb_count = reinterpret_cast<unsigned *>(h->d_partial + 2 * nl::kClipSlots);
        a.partial = h->d_partial;
        a.final = h->d_counters;
        a.zero_next = h->d_sets + (size_t)(h->cur_set ^ 1) * nl::kScratchWords;
    } else if (!h->partial_clean) {
        NL_HIP(hipMemsetAsync(h->d_partial, 0, kScratchBytes, h->stream));
    }
    h->sets_clean = false;                       // until this pass is enqueued completely
    const bool keep_clean = h->partial_clean && mode == NL_ST_MEAN;     // (a mean pass does not touch the scratch set)
    h->partial_clean = false;
    if (timed && !one_start) NL_HIP(hipEventRecord(h->ev_dom0, h->stream));

    const nl::Form form = maps ? nl::Form::Maps : (wclip || wmad) ? nl::Form::Follow : nl::Form::Plain;
    const PassSetup p{mode, weighted, timed, fused, a, form};
    PassFacts facts;
    int rc = NL_OK;
    switch (engine) {
    case Engine::Mean:            rc = run_mean(h, p, &facts); break;
    case Engine::MedianRegisters: rc = run_median(h, p, false); break;
    case Engine::MedianMultiLane: rc = run_median(h, p, true); break;
    case Engine::Listed:          rc = run_listed(h, p, &facts); break;
    case Engine::SigmaFast:       rc = run_sigma_fast(h, p, &facts); break;
    case Engine::SigmaMaps:       rc = run_sigma_maps(h, p, &facts); break;
    case Engine::WeightedTile:    rc = run_weighted_tile(h, p, &facts); break;
    case Engine::DenseReplay:     rc = run_dense_replay(h, p, &facts); break;
    case Engine::ExactColumns:    rc = run_exact_columns(h, p, &facts); break;
    case Engine::LinfitWeighted:  rc = run_linfit_weighted(h, p, &facts); break;
    case Engine::ClipWeighted:    rc = run_clip_weighted(h, p, &facts); break;
    case Engine::MadWeighted:     rc = run_mad_weighted(h, p, &facts); break;
    case Engine::DeepMedian:      rc = run_deep_median(h, p); break;
    case Engine::DeepMad:         rc = run_deep_mad(h, p, &facts); break;
    case Engine::DeepMadWeighted: rc = run_deep_mad_weighted(h, p, &facts); break;
    }
    if (rc != NL_OK) return rc;
    NL_HIP(hipEventRecord(h->ev_stop, h->stream));
    h->last = facts;
    h->sets_clean = facts.fused;
    h->partial_clean = facts.zeroed_behind || keep_clean;
    h->pass_seq++;
    h->last_mode = mode;
    h->last_maps = maps;
    h->pending = true;
    return NL_OK;
}

int nl_stack_finish(nl_stack_t *h, float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    NL_CHECK_HANDLE(h);
    unsigned long long c[4] = {0, 0, 0, 0};
    // (a fast sigma / winsorized pass leaves its list lengths behind the totals: c[2] = exact list | generic list << 32)
    if (h->last.has_counters && (clip_low || clip_high || h->last.lists))
        NL_HIP(hipMemcpyAsync(c, h->d_counters, h->last.lists ? 3 * sizeof c[0] : 2 * sizeof c[0], hipMemcpyDeviceToHost, h->stream));
    if (out_host)
        NL_HIP(hipMemcpyAsync(out_host + (int64_t)h->row0 * h->width, h->d_out,
                              (size_t)h->npix * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    h->pending = false;
    if (h->last.has_counters && h->last.lists) {
        h->fb_hint = (unsigned)(c[2] & 0xffffffffull) + 1u;
        h->gen_hint = (unsigned)(c[2] >> 32) + 1u;
        hints_store({h->n_frames, h->npix, h->last_mode, h->last_weighted}, h->fb_hint, h->gen_hint);
    }
    if (clip_low) *clip_low = (int64_t)c[0];
    if (clip_high) *clip_high = (int64_t)c[1];
    return NL_OK;
}

}  // extern "C"

// nl_stack_finish, and the two planes of the map (of either kind of maps pass).  The packed words come down in ONE copy and are split here: the same
// bytes cross the link as two uint16 planes would, and no second device buffer or kernel exists for what is a 16-bit
// shuffle beside a PCIe transfer.
static int stack_finish_maps(nl_stack_t *h, float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host,
                             uint16_t *reject_high_host)
{
    NL_CHECK_HANDLE(h);
    if (!h->last_maps || !h->d_reject_map) return fail(NL_ERR_INVALID_ARG, "finish_maps: the last pass was no maps pass");
    std::vector<unsigned> packed;
    if (reject_low_host || reject_high_host) {
        packed.resize((size_t)h->npix);
        // (enqueued in front of nl_stack_finish's own copies; its synchronize covers this one)
        NL_HIP(hipMemcpyAsync(packed.data(), h->d_reject_map, (size_t)h->npix * sizeof(unsigned), hipMemcpyDeviceToHost, h->stream));
    }
    const int rc = nl_stack_finish(h, out_host, clip_low, clip_high);
    if (rc != NL_OK) {
        (void)hipStreamSynchronize(h->stream);          // (the copy into `packed` may still be in flight)
        return rc;
    }
    const int64_t at = (int64_t)h->row0 * h->width;
    if (reject_low_host)
        for (int64_t i = 0; i < h->npix; i++) reject_low_host[at + i] = (uint16_t)(packed[(size_t)i] & 0xffffu);
    if (reject_high_host)
        for (int64_t i = 0; i < h->npix; i++) reject_high_host[at + i] = (uint16_t)(packed[(size_t)i] >> 16);
    return NL_OK;
}

// ---- the two halves of a pass, and the pass entries of the handle as forwards to them ----------
int nl::stack_start(nl_stack_t *h, const nl::PassRequest &req) { return settle_failed_pass(h, run_async_impl(h, req)); }

int nl::stack_finish(nl_stack_t *h, const nl::PassRequest &req, const nl::PassOutputs &to)
{
    if (req.tier == nl::MapsTier::None) return nl_stack_finish(h, to.out, to.clip_low, to.clip_high);
    return stack_finish_maps(h, to.out, to.clip_low, to.clip_high, to.reject_low, to.reject_high);
}

static int run_pass(nl_stack_t *h, const nl::PassRequest &req, const nl::PassOutputs &to)
{
    const int rc = nl::stack_start(h, req);
    return rc != NL_OK ? rc : nl::stack_finish(h, req, to);
}

// what nl_stack_run_clip_weighted* can tell from the mode alone, in front of the handle (NL_ST_AUTO is resolved behind it)
static int clip_weighted_mode_check(int mode)
{
    if (mode < NL_ST_MEDIAN || mode > NL_ST_AUTO) return fail(NL_ERR_INVALID_MODE, "invalid stacking mode");
    if (mode != NL_ST_AUTO && mode != NL_ST_SIGMA && mode != NL_ST_WINSOR_SIGMA)
        return fail(NL_ERR_INVALID_MODE, "run_clip_weighted: mode %d is neither NL_ST_SIGMA nor NL_ST_WINSOR_SIGMA", mode);
    return NL_OK;
}

extern "C" {

int nl_stack_run_async(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc)
{
    return nl::stack_start(h, {PassKind::Default, MapsTier::None, mode, sigma_low, sigma_high, ref_loc});
}

int nl_stack_run(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                 float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    return run_pass(h, {PassKind::Default, MapsTier::None, mode, sigma_low, sigma_high, ref_loc}, {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the weighted linear-fit pass (include/nlstack_wlinfit.h)
int nl_stack_run_linfit_weighted_async(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc)
{
    return nl::stack_start(h, {PassKind::WeightedLinfit, MapsTier::None, NL_ST_LINEAR_FIT, sigma_low, sigma_high, ref_loc});
}

int nl_stack_run_linfit_weighted(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc,
                                 float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    return run_pass(h, {PassKind::WeightedLinfit, MapsTier::None, NL_ST_LINEAR_FIT, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the weighted clip pass whose weights follow their frames (include/nlstack_wclip.h)
int nl_stack_run_clip_weighted_async(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc)
{
    const int rc = clip_weighted_mode_check(mode);
    return rc != NL_OK ? rc : nl::stack_start(h, {PassKind::WeightedClip, MapsTier::None, mode, sigma_low, sigma_high, ref_loc});
}

int nl_stack_run_clip_weighted(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    const int rc = clip_weighted_mode_check(mode);
    return rc != NL_OK ? rc
                       : run_pass(h, {PassKind::WeightedClip, MapsTier::None, mode, sigma_low, sigma_high, ref_loc},
                                  {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the weighted MAD-sigma pass (include/nlstack_wmad.h)
int nl_stack_run_mad_weighted_async(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc)
{
    return nl::stack_start(h, {PassKind::WeightedMad, MapsTier::None, NL_ST_MAD_SIGMA, sigma_low, sigma_high, ref_loc});
}

int nl_stack_run_mad_weighted(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc,
                              float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    return run_pass(h, {PassKind::WeightedMad, MapsTier::None, NL_ST_MAD_SIGMA, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the deep pass (include/nlstack_deepstack.h)
int nl_stack_run_deepstack_async(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc)
{
    return nl::stack_start(h, {PassKind::DeepStack, MapsTier::None, mode, sigma_low, sigma_high, ref_loc});
}

int nl_stack_run_deepstack(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    return run_pass(h, {PassKind::DeepStack, MapsTier::None, mode, sigma_low, sigma_high, ref_loc}, {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the deep weighted MAD-sigma pass (include/nlstack_deepwmad.h)
int nl_stack_run_mad_weighted_deepstack_async(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc)
{
    return nl::stack_start(h, {PassKind::DeepWeightedMad, MapsTier::None, NL_ST_MAD_SIGMA, sigma_low, sigma_high, ref_loc});
}

int nl_stack_run_mad_weighted_deepstack(nl_stack_t *h, float sigma_low, float sigma_high, float ref_loc,
                                        float *out_host, int64_t *clip_low, int64_t *clip_high)
{
    return run_pass(h, {PassKind::DeepWeightedMad, MapsTier::None, NL_ST_MAD_SIGMA, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, nullptr, nullptr});
}

// the maps passes (include/nlstack_maps.h, nlstack_fastmaps.h, nlstack_residentmaps.h, nlstack_deepmaps.h, nlstack_fullmaps.h,
// nlstack_deepstackmaps.h): one tier each
int nl_stack_run_maps(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                      float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    return run_pass(h, {PassKind::Default, MapsTier::Column, mode, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_stack_run_maps_fast(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    return run_pass(h, {PassKind::Default, MapsTier::Fast, mode, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_stack_run_maps_resident(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                               float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    return run_pass(h, {PassKind::Default, MapsTier::Resident, mode, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_stack_run_maps_deep(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    return run_pass(h, {PassKind::Default, MapsTier::Deep, mode, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_stack_run_maps_full(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                           float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    return run_pass(h, {PassKind::Default, MapsTier::Full, mode, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

int nl_stack_run_maps_deepstack(nl_stack_t *h, int mode, float sigma_low, float sigma_high, float ref_loc,
                                float *out_host, int64_t *clip_low, int64_t *clip_high, uint16_t *reject_low_host, uint16_t *reject_high_host)
{
    return run_pass(h, {PassKind::Default, MapsTier::DeepStack, mode, sigma_low, sigma_high, ref_loc},
                    {out_host, clip_low, clip_high, reject_low_host, reject_high_host});
}

// no pass: it reads the active frames behind whatever is enqueued on the handle's stream and leaves the last pass's
// result, mode, kernel name and bookkeeping alone
int nl_stack_coverage(nl_stack_t *h, uint16_t *coverage_host)
{
    NL_CHECK_HANDLE(h);
    if (!coverage_host) return fail(NL_ERR_INVALID_ARG, "coverage: null output");
    if (h->n_frames > 65535)
        return fail(NL_ERR_TOO_MANY_FRAMES, "coverage: %d active frames, a uint16 map holds counts up to 65535", h->n_frames);
    if (h->uploads_pending) {
        // asynchronous uploads: wait for the last DMA on the device, as a pass does
        const int last = (h->stage_next + kStageSlots - 1) % kStageSlots;
        NL_HIP(hipStreamWaitEvent(h->stream, h->stage_done[last], 0));
        h->uploads_pending = false;
    }
    if (!h->d_coverage) NL_HIP(dev_malloc(&h->d_coverage, (size_t)h->npix * sizeof(uint16_t)));
    if (!h->ev_cov0) {
        NL_HIP(hipEventCreateWithFlags(&h->ev_cov0, hipEventDefault | h->ev_rel));
        NL_HIP(hipEventCreateWithFlags(&h->ev_cov1, hipEventDefault | h->ev_rel));
    }
    NL_HIP(hipEventRecord(h->ev_cov0, h->stream));
    NL_HIP(nl::launch_stack_coverage(h->d_frames, h->fstride, h->npix, h->n_frames, h->d_coverage, h->stream));
    NL_HIP(hipEventRecord(h->ev_cov1, h->stream));
    NL_HIP(hipMemcpyAsync(coverage_host + (int64_t)h->row0 * h->width, h->d_coverage, (size_t)h->npix * sizeof(uint16_t),
                          hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// GPU time from event `from` to event `to` of the last pass, once `to` has completed; -1 where unavailable
static float elapsed_ms(nl_stack_t *h, hipEvent_t from, hipEvent_t to)
{
    float ms = -1.0f;
    if (hipSetDevice(h->device) != hipSuccess || hipEventSynchronize(to) != hipSuccess ||
        hipEventElapsedTime(&ms, from, to) != hipSuccess)
        return -1.0f;
    return ms;
}

float nl_stack_last_coverage_ms(nl_stack_t *h) { return h && h->ev_cov0 ? elapsed_ms(h, h->ev_cov0, h->ev_cov1) : -1.0f; }
float nl_stack_last_dominant_kernel_ms(nl_stack_t *h) { return h && h->ev_dom0 ? elapsed_ms(h, h->ev_dom0, h->ev_dom1) : -1.0f; }

int nl_stack_set_exact(nl_stack_t *h, int on)
{
    NL_CHECK_HANDLE(h);
    if (on < 0 || on > 4) return fail(NL_ERR_INVALID_ARG, "set_exact: unknown flavour %d (0 ... 4)", on);
    // (a switch whose code was removed must not fall through to another kernel silently: an A/B run would time the same
    // kernel twice)
    if (on == 4)
        return fail(NL_ERR_INVALID_ARG, "set_exact: flavour 4 (four pixels per wave) was removed with the experiments build");
    h->force_exact = on != 0;
    h->exact_flavour = on;
    return NL_OK;
}

int nl_stack_set_dev_flags(nl_stack_t *h, unsigned flags)
{
    NL_CHECK_HANDLE(h);
    if (flags & kDevRemovedPasses)
        return fail(NL_ERR_INVALID_ARG, "set_dev_flags: switches 1024 / 2048 (split / persistent LDS-column pass) were removed with the "
                                        "experiments build");
    h->dev_flags = flags;
    return NL_OK;
}

// list lengths of the last fast pass: a sigma / winsorized pass leaves them behind its totals (d_counters[2] = exact list |
// generic list << 32 -- its own counters may be zeroed again by then), the other fast passes keep them in the scratch set
static int64_t last_list_length(nl_stack_t *h, int which)
{
    if (hipSetDevice(h->device) != hipSuccess) return -1;
    if (h->last.lists) {
        unsigned long long c = 0;
        if (hipMemcpyAsync(&c, h->d_counters + 2, sizeof c, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
        if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
        return which == 0 ? (int64_t)(c & 0xffffffffull) : (int64_t)(c >> 32);
    }
    unsigned c = 0;
    if (hipMemcpyAsync(&c, h->d_fb_count + which, sizeof c, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    return (int64_t)c;
}

int64_t nl_stack_last_fallback_pixels(nl_stack_t *h)
{
    if (!h || !h->last.used_fast || !h->d_fb_count) return 0;
    return last_list_length(h, 0);
}

int nl_stack_last_pass_protocol(nl_stack_t *h)
{
    if (!h) return 0;
    return (h->last.fused ? 1 : 0) | (h->last.tail_fused ? 2 : 0);
}

int64_t nl_stack_last_generic_pixels(nl_stack_t *h)
{
    if (!h || !h->last.used_fast || !h->d_fb_count || !h->d_gen_list) return 0;
    return last_list_length(h, 1);
}

int nl_stack_linfit_stage_counts(nl_stack_t *h, unsigned *counts, int n)
{
    if (!h || !counts || n <= 0 || !h->d_lf_count || h->last_mode != NL_ST_LINEAR_FIT || !h->last.used_fast) return 0;
    if (hipSetDevice(h->device) != hipSuccess) return -1;
    unsigned c[nl::kLinfitCounters] = {};
    if (hipMemcpyAsync(c, h->d_lf_count, sizeof c, hipMemcpyDeviceToHost, h->stream) != hipSuccess) return -1;
    if (hipStreamSynchronize(h->stream) != hipSuccess) return -1;
    const int m = n < nl::kLinfitCounters ? n : nl::kLinfitCounters;
    for (int i = 0; i < m; i++) counts[i] = c[i];
    return m;
}

// GPU times of a pass that is `back` passes old (0 = the last one enqueued); -1 where unavailable
int nl_stack_pass_times(nl_stack_t *h, int back, float *pass_ms, float *dominant_ms)
{
    NL_CHECK_HANDLE(h);
    if (back < 0 || back >= kTimingRing || (int64_t)back >= h->pass_seq)
        return fail(NL_ERR_INVALID_ARG, "pass_times: pass %d back is not in the ring of %d", back, kTimingRing);
    const int slot = (int)((h->pass_seq - 1 - back) % kTimingRing);
    if (!h->ring_timed[slot])
        return fail(NL_ERR_INVALID_ARG, "pass_times: pass %d back ran without timing events (developer switch 32)", back);
    NL_HIP(hipEventSynchronize(h->ring_stop[slot]));
    float ms = -1.0f;
    if (pass_ms) {
        NL_HIP(hipEventElapsedTime(&ms, h->ring_start[slot], h->ring_stop[slot]));
        *pass_ms = ms;
    }
    if (dominant_ms) {
        NL_HIP(hipEventElapsedTime(&ms, h->ring_dom0_is_start[slot] ? h->ring_start[slot] : h->ring_dom0[slot], h->ring_dom1[slot]));
        *dominant_ms = ms;
    }
    return NL_OK;
}

// enqueues, behind the last pass on the handle's stream, a 16-byte device-to-device copy of its
// {clip_low, clip_high} totals into a caller-owned device buffer (e.g. the tensor an RCCL
// all-reduce runs on): no host round trip between the pass and the reduction
int nl_stack_copy_counters_async(nl_stack_t *h, void *device_dst)
{
    NL_CHECK_HANDLE(h);
    if (!device_dst) return fail(NL_ERR_INVALID_ARG, "copy_counters_async: null destination");
    if (h->last.has_counters)
        NL_HIP(hipMemcpyAsync(device_dst, h->d_counters, 2 * sizeof(unsigned long long), hipMemcpyDeviceToDevice, h->stream));
    else
        NL_HIP(hipMemsetAsync(device_dst, 0, 2 * sizeof(unsigned long long), h->stream));
    return NL_OK;
}

void *nl_stack_stream(nl_stack_t *h) { return h ? (void *)h->stream : nullptr; }
void *nl_stack_counters_device_ptr(nl_stack_t *h) { return h ? (void *)h->d_counters : nullptr; }

int nl_stack_set_counters_buffer(nl_stack_t *h, void *device_buf)
{
    NL_CHECK_HANDLE(h);
    h->d_counters = device_buf ? static_cast<unsigned long long *>(device_buf) : h->d_counters_own;
    return NL_OK;
}

int nl_stack_order_stream_after(nl_stack_t *h, void *hip_stream)
{
    NL_CHECK_HANDLE(h);
    if (!hip_stream) return fail(NL_ERR_INVALID_ARG, "order_stream_after: null stream");
    // a ring of events: the waiting stream may still be working off an older one when the next pass is enqueued
    const int slot = h->order_seq++ % kOrderRing;
    if (!h->ev_order[slot]) NL_HIP(hipEventCreateWithFlags(&h->ev_order[slot], hipEventDisableTiming | h->ev_rel));
    NL_HIP(hipEventRecord(h->ev_order[slot], h->stream));
    NL_HIP(hipStreamWaitEvent(static_cast<hipStream_t>(hip_stream), h->ev_order[slot], 0));
    return NL_OK;
}

float nl_stack_last_kernel_ms(nl_stack_t *h) { return h && h->ev_start ? elapsed_ms(h, h->ev_start, h->ev_stop) : -1.0f; }

// stackfindsigma.go:48-98 (commented-out reference code = the spec)
int nl_stack_find_sigmas(nl_stack_t *h, int mode, float ref_loc,
                         float clip_perc_low, float clip_perc_high,
                         nl_reduce_fn reduce, void *user,
                         float *out_host, int64_t *clip_low, int64_t *clip_high,
                         float *sigma_low, float *sigma_high, int *passes)
{
    NL_CHECK_HANDLE(h);
    if (mode == NL_ST_AUTO) mode = nl::auto_select_mode(h->n_frames);
    if (mode < NL_ST_MEDIAN || mode > NL_ST_LINEAR_FIT) return fail(NL_ERR_INVALID_MODE, "invalid stacking mode");
    // the counters cover the samples the percentages are taken of: with a reducer the whole
    // image (every tile contributes), without one only this handle's tile
    const int64_t total = reduce ? (int64_t)h->width * h->height * (int64_t)h->n_frames
                                 : h->npix * (int64_t)h->n_frames;
    return nl::goal_seek(
        mode, clip_perc_low, clip_perc_high, total,
        [&](float lo, float hi, int64_t c[2]) {          // (with a reducer: c over every tile)
            int rc = nl_stack_run(h, mode, lo, hi, ref_loc, nullptr, &c[0], &c[1]);
            if (rc != NL_OK) return rc;
            if (reduce && (rc = reduce(c, user)) != 0)
                return fail(NL_ERR_INVALID_ARG, "counter reduction callback failed (%d)", rc);
            return NL_OK;
        },
        [&](float lo, float hi) { return nl_stack_run(h, mode, lo, hi, ref_loc, nullptr, nullptr, nullptr); },
        [&] { return out_host ? nl_stack_finish(h, out_host, nullptr, nullptr) : NL_OK; },
        {clip_low, clip_high, sigma_low, sigma_high, passes});
}

// StackIncremental / StackIncrementalFinalize, stack.go:924-944
int nl_stack_accumulate(nl_stack_t *h, float weight, int first)
{
    NL_CHECK_HANDLE(h);
    if (!h->d_acc) NL_HIP(dev_malloc(&h->d_acc, (size_t)h->npix * sizeof(float)));
    NL_HIP(nl::launch_axpy(h->d_acc, h->d_out, weight, first, h->npix, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl_stack_accumulate_finalize(nl_stack_t *h, float weight_sum, float *out_host)
{
    NL_CHECK_HANDLE(h);
    if (!h->d_acc) return fail(NL_ERR_INVALID_ARG, "accumulate_finalize before accumulate");
    volatile float factor = 1.0f / weight_sum;
    NL_HIP(nl::launch_scale(h->d_acc, factor, h->npix, h->stream));
    if (out_host)
        NL_HIP(hipMemcpyAsync(out_host + (int64_t)h->row0 * h->width, h->d_acc,
                              (size_t)h->npix * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

}  // extern "C"
