// nlstack_api.hip -- the C ABI of libnlstack.so (include/nlstack.h): error state, the device-memory cache, the pinned
// staging pool and the stream pool; handle create / destroy / attach / weights / accessors; every upload and download,
// FITS and projected ingest included.  Stack passes: nlstack_pass.hip; steps on one resident frame: nlstack_frame.hip
// (statistics, median filters, projection) and, by the reference command they serve, nlstack_frame_pre.hip,
// nlstack_frame_stretch.hip and nlstack_frame_rgb.hip; what all share: nlstack_internal.hpp.  There is no CPU fallback:
// without a HIP device every compute entry point fails with NL_ERR_NO_DEVICE / NL_ERR_HIP.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include <mutex>
#include <thread>

#include "nlstack_internal.hpp"

thread_local std::string nl::g_err;

int nl::fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// the thread's error message, for the other translation units of the library (nlstack_group.hip)
namespace nl { void set_last_error(const char *msg) { g_err = msg ? msg : ""; } }

namespace {

constexpr int kStageThreads = 4;    // host threads filling one staging buffer

// ---- device-memory cache ---------------------------------------------------------------------------------------------
// The cgo drop-in creates a handle per OpStack.Apply (stack.go:131-138 allocates per call as well) and destroys it
// afterwards: hipMalloc + hipFree of the frame buffer alone cost more than the headline pass (measured, bench.py
// "fresh_handle": create 1.0 - 1.6 ms, destroy 1.3 - 1.8 ms, pass 1.7 ms).  The large buffers of a destroyed handle are
// therefore parked -- per device at most kCacheBlocks of them and NL_MEM_CACHE_MB MiB (default: a sixteenth of the device's memory; 0 = off) -- and the
// next handle with the same sizes on the same device takes them over.  nl_release_cached_memory() returns them to HIP.
constexpr int kCacheBlocks = 64;
constexpr size_t kCacheMinBytes = (size_t)1 << 20;
struct CachedBlock { int device; size_t bytes; void *ptr; };
std::mutex g_cache_mu;
std::vector<CachedBlock> g_cache;
size_t g_cache_bytes = 0;

// Limit of the parked bytes: NL_MEM_CACHE_MB if set (0 = off), else a sixteenth of the device's memory (18 GB of an
// MI355X's 288: the frame buffer of the headline stack is 8 GiB) -- blocks parked by this library are invisible to the
// other allocators of the process (torch, RCCL) until an allocation of OURS fails, so the default stays small.
size_t cache_limit(int device = -1)
{
    static const long long env_mb = [] { const char *e = getenv("NL_MEM_CACHE_MB"); return e ? atoll(e) : -1ll; }();
    if (env_mb >= 0) return env_mb > 0 ? (size_t)env_mb << 20 : (size_t)0;
    // a sixteenth of THAT device's memory (a table per device: the limit used to be whatever device was current at the
    // first free, applied to all)
    static std::mutex mu;
    static std::vector<size_t> per_device;
    std::lock_guard<std::mutex> lk(mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    if (device < 0) device = cur;
    if ((size_t)device >= per_device.size()) per_device.resize((size_t)device + 1, 0);
    if (per_device[(size_t)device] == 0) {
        size_t free_b = 0, total_b = 0;
        if (device != cur) (void)hipSetDevice(device);
        const bool ok = hipMemGetInfo(&free_b, &total_b) == hipSuccess;
        if (!ok) (void)hipGetLastError();
        if (device != cur) (void)hipSetDevice(cur);
        per_device[(size_t)device] = ok ? total_b / 16 : (size_t)4096 << 20;
    }
    return per_device[(size_t)device];
}

void cache_release_all()
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const CachedBlock &b : g_cache) {
        (void)hipSetDevice(b.device);
        (void)hipFree(b.ptr);
    }
    g_cache.clear();
    g_cache_bytes = 0;
    (void)hipSetDevice(cur);
}

}  // namespace

// EVERY device allocation of the library goes through here: when HIP is out of memory while blocks are parked, they are
// handed back and the allocation is tried again (the caller has selected the device).
hipError_t nl::dev_malloc(void **p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if (e == hipSuccess) return e;
    bool parked;
    { std::lock_guard<std::mutex> lk(g_cache_mu); parked = !g_cache.empty(); }
    if (!parked) return e;
    (void)hipGetLastError();
    cache_release_all();
    return hipMalloc(p, bytes);
}

// (the caller has selected `device`)
hipError_t nl::cached_malloc(void **p, size_t bytes, int device)
{
    if (bytes >= kCacheMinBytes) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        for (size_t i = 0; i < g_cache.size(); i++)
            if (g_cache[i].device == device && g_cache[i].bytes == bytes) {
                *p = g_cache[i].ptr;
                g_cache_bytes -= bytes;
                g_cache.erase(g_cache.begin() + (long)i);
                return hipSuccess;
            }
    }
    return dev_malloc(p, bytes);
}

void nl::cached_free(void *p, size_t bytes, int device)
{
    if (!p) return;
    if (bytes >= kCacheMinBytes) {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        // (both limits per DEVICE: a group of one tile per GPU parks the buffers of all its tiles, nlstack_group.hip)
        int blocks = 0;
        size_t parked = 0;
        for (const CachedBlock &b : g_cache)
            if (b.device == device) { blocks++; parked += b.bytes; }
        static const int max_blocks = [] { const char *e = getenv("NL_CACHE_BLOCKS"); return e ? atoi(e) : kCacheBlocks; }();
        if (blocks < max_blocks && parked + bytes <= cache_limit(device)) {
            g_cache.push_back({device, bytes, p});
            g_cache_bytes += bytes;
            return;
        }
    }
    (void)hipFree(p);
}

hipError_t nl::DevBuffer::reserve(size_t want, hipStream_t stream)
{
    if (want <= bytes) return hipSuccess;
    if (ptr) {
        const hipError_t e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        release();
    }
    const hipError_t e = dev_malloc(&ptr, want);
    if (e != hipSuccess) ptr = nullptr;
    else bytes = want;
    return e;
}

namespace {

// Pinned staging buffers are parked as well (round 6): a handle per Apply allocated its ring of kStageSlots pinned buffers
// inside its first uploads and freed it in destroy -- hipHostMalloc + hipHostFree of 4 x 64 MiB are 10 + 10 ms of the 180 ms an
// Apply of 128 frames from host memory takes (bench.py apply_from_host).  At most kPinnedBlocks blocks / kPinnedLimit bytes
// stay (process-wide: pinned memory belongs to no device); a request takes the smallest parked block that is large enough.
constexpr size_t kPinnedBlocks = 16;
constexpr size_t kPinnedLimit = (size_t)2 << 30;
std::mutex g_pinned_mu;
std::vector<std::pair<size_t, void *>> g_pinned;
size_t g_pinned_bytes = 0;

hipError_t pinned_malloc(void **p, size_t bytes, size_t *cap)
{
    {
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        size_t best = g_pinned.size();
        for (size_t i = 0; i < g_pinned.size(); i++)
            if (g_pinned[i].first >= bytes && (best == g_pinned.size() || g_pinned[i].first < g_pinned[best].first)) best = i;
        if (best < g_pinned.size() && g_pinned[best].first <= 2 * bytes + ((size_t)1 << 20)) {
            *p = g_pinned[best].second;
            *cap = g_pinned[best].first;
            g_pinned_bytes -= g_pinned[best].first;
            g_pinned.erase(g_pinned.begin() + (long)best);
            return hipSuccess;
        }
    }
    *cap = bytes;
    return hipHostMalloc(p, bytes, hipHostMallocDefault);
}

void pinned_free(void *p, size_t cap)
{
    if (!p) return;
    if (cache_limit() > 0) {                               // (NL_MEM_CACHE_MB=0 turns every cache of the library off)
        std::lock_guard<std::mutex> lk(g_pinned_mu);
        if (g_pinned.size() < kPinnedBlocks && g_pinned_bytes + cap <= kPinnedLimit) {
            g_pinned.emplace_back(cap, p);
            g_pinned_bytes += cap;
            return;
        }
    }
    (void)hipHostFree(p);
}

void pinned_release_all()
{
    std::lock_guard<std::mutex> lk(g_pinned_mu);
    for (const auto &e : g_pinned) (void)hipHostFree(e.second);
    g_pinned.clear();
    g_pinned_bytes = 0;
}

// Streams are parked like the buffers: destroying the two or three streams of a handle is most of what nl_stack_destroy
// costs once the buffers stay (tools/group_create_probe.py), and the drop-in makes a handle per Apply.  A parked stream is idle
// (synchronised before it is parked); nl_release_cached_memory destroys them.
// A stream keeps its ROLE (round 6): HIP binds a stream to one of its few hardware queues when it is created, and the main and
// side stream of a handle -- created back to back -- sit on different ones, which is what lets the replay of a pass run beside its
// generic pass.  Round 5 parked all streams in one list: the next handle's main stream could be a former copy stream (created
// lazily, any queue) next to a former side stream on the SAME queue, and the tail of every pass with a long replay serialised
// (C3 tile 4.10 -> 4.58 ms, winsor 24 2.65 -> 2.88, tools/bisect_tail.sh, profiles/r06_bisect_tail.txt).  Main + side are
// therefore parked and handed out as the PAIR they were created as; copy streams have a list of their own.
// NL_STREAM_POOL=0 turns the pool off.
constexpr size_t kStreamPool = 32;
struct StreamPair { int device; hipStream_t main, side; };
std::mutex g_stream_mu;
std::vector<StreamPair> g_stream_pairs;
std::vector<std::pair<int, hipStream_t>> g_copy_streams;           // (device, non-blocking stream at default priority)

bool stream_pool_on()
{
    static const bool on = [] { const char *e = getenv("NL_STREAM_POOL"); return !e || atoi(e) != 0; }();
    return on;
}

hipError_t pooled_stream_pair(hipStream_t *main, hipStream_t *side, int device)
{
    if (stream_pool_on()) {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        for (size_t i = g_stream_pairs.size(); i-- > 0;)
            if (g_stream_pairs[i].device == device) {
                *main = g_stream_pairs[i].main;
                *side = g_stream_pairs[i].side;
                g_stream_pairs.erase(g_stream_pairs.begin() + (long)i);
                return hipSuccess;
            }
    }
    hipError_t e = hipStreamCreateWithFlags(main, hipStreamNonBlocking);
    if (e != hipSuccess) return e;
    e = hipStreamCreateWithFlags(side, hipStreamNonBlocking);
    if (e != hipSuccess) { (void)hipStreamDestroy(*main); *main = nullptr; }
    return e;
}

hipError_t pooled_copy_stream(hipStream_t *s, int device)
{
    if (stream_pool_on()) {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        for (size_t i = g_copy_streams.size(); i-- > 0;)
            if (g_copy_streams[i].first == device) {
                *s = g_copy_streams[i].second;
                g_copy_streams.erase(g_copy_streams.begin() + (long)i);
                return hipSuccess;
            }
    }
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

static bool stream_idle(hipStream_t s)
{
    if (hipStreamSynchronize(s) == hipSuccess) return true;
    (void)hipGetLastError();
    return false;
}

void park_stream_pair(hipStream_t main, hipStream_t side, int device)
{
    if (main && side && stream_pool_on() && stream_idle(side) && stream_idle(main)) {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        size_t n = 0;
        for (const auto &e : g_stream_pairs) n += e.device == device;
        if (n < kStreamPool / 2) { g_stream_pairs.push_back({device, main, side}); return; }
    }
    if (side) (void)hipStreamDestroy(side);
    if (main) (void)hipStreamDestroy(main);
}

void park_copy_stream(hipStream_t s, int device)
{
    if (!s) return;
    if (stream_pool_on() && stream_idle(s)) {
        std::lock_guard<std::mutex> lk(g_stream_mu);
        size_t n = 0;
        for (const auto &e : g_copy_streams) n += e.first == device;
        if (n < kStreamPool / 2) { g_copy_streams.emplace_back(device, s); return; }
    }
    (void)hipStreamDestroy(s);
}

void stream_pool_release_all()
{
    std::lock_guard<std::mutex> lk(g_stream_mu);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (const auto &e : g_copy_streams) { (void)hipSetDevice(e.first); (void)hipStreamDestroy(e.second); }
    g_copy_streams.clear();
    for (const auto &e : g_stream_pairs) { (void)hipSetDevice(e.device); (void)hipStreamDestroy(e.side); (void)hipStreamDestroy(e.main); }
    g_stream_pairs.clear();
    (void)hipSetDevice(cur);
}

}  // namespace

// stats.MeanStdDev over xs = 0..n-1 (stats.go:246-261, called from :570) depends on n only: tabulated once per frame count
// of the process, in the same fp32 operation order ({mean, stddev} for n = 1 .. n_frames at [2n], [2n + 1]).  (The table is
// O(n^2) scalar operations: 0.45 ms of a 512-frame handle's create.)  Returned by value: 8 bytes per frame.
static std::vector<float> xstat_table(int n_frames)
{
    static std::mutex mu;
    static std::vector<std::pair<int, std::vector<float>>> tables;        // (a handful of frame counts per process)
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &t : tables)
        if (t.first == n_frames) return t.second;
    std::vector<float> xstat(2 * (size_t)(n_frames + 1), 0.0f);
    for (int n = 1; n <= n_frames; n++) {
        volatile float s = 0.0f;
        for (int i = 0; i < n; i++) s = s + (float)i;
        const float mean = s / (float)n;
        volatile float v = 0.0f;
        for (int i = 0; i < n; i++) {
            volatile float d = (float)i - mean;
            volatile float dd = d * d;
            v = v + dd;
        }
        const float var = v / (float)n;
        xstat[2 * (size_t)n] = mean;
        xstat[2 * (size_t)n + 1] = (float)sqrt((double)var);
    }
    if (tables.size() >= 64) tables.erase(tables.begin());
    tables.emplace_back(n_frames, xstat);
    return xstat;
}

// Floats between consecutive frames of the owned planar buffer.  A stride that is a multiple of a large power of two
// -- 4096 x 4096 floats = 2^26 bytes, or a 512-row tile's 2^23 -- puts the same pixel of every frame into the same
// HBM channel / bank: the 4 frames one load of the LDS-column kernels reads, and the 128-512 loads a wave has in
// flight, then queue on a few banks while the rest idle.  Measured on sigma 512 x 4096^2 (profiles/r05_stride_pad.txt):
// stride + 0: 10.9 ms, + 16 KiB: 10.6, + 32 KiB: 10.2, + 64 KiB: 9.75, + 64 KiB + 256 B: 9.60, more: no further gain;
// 32 frames are indifferent, 128 frames gain 1-3 %.  So the frame is rounded up to 128 KiB and 64 KiB + 256 B are added:
// the residue of the stride modulo 128 KiB is the measured optimum for every tile size, at a cost of at most 192 KiB
// per frame.  Small tiles (< 1 MiB per frame) are left dense.  NL_STRIDE_PAD=<floats> (developer) sets the padding
// added to the tile's pixel count instead (0 = the dense layout of rounds 1-4).
static bool frame_stride_addressable(int64_t npix, int64_t stride)
{
    // pixel offset + 3 frames in one signed 32-bit byte offset (multi-lane gathers), stride a multiple of 16 bytes
    // where the dense layout is one (the float4 loads of the mean and the replay kernels)
    return (npix + 3 * stride) * 4 < ((int64_t)1 << 31) && (npix % 4 != 0 || stride % 4 == 0);
}

static int64_t padded_frame_stride(int64_t npix)
{
    const char *e = getenv("NL_STRIDE_PAD");                  // read per handle: the tests switch it
    const long env_pad = e ? atol(e) : -1L;
    int64_t stride = npix;
    if (env_pad >= 0) stride = npix + env_pad;
    else if (npix >= (1 << 18)) stride = ((npix + 32767) & ~(int64_t)32767) + 16384 + 64;
    if (stride != npix && npix < nl::kFastMaxPixels && !frame_stride_addressable(npix, stride)) stride = npix;
    return stride;
}

int nl::require_device(int *count)
{
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(NL_ERR_NO_DEVICE, "no HIP device available (%s); libnlstack has no CPU path", hipGetErrorString(e));
    if (count) *count = ndev;
    return NL_OK;
}

int nl::select_device(int device)
{
    int ndev = 0;
    const int rc = require_device(&ndev);
    if (rc != NL_OK) return rc;
    if (device < 0 || device >= ndev) return fail(NL_ERR_INVALID_ARG, "device %d out of range (have %d)", device, ndev);
    NL_HIP(hipSetDevice(device));
    return NL_OK;
}

namespace nl {

// internal/star/coord.go:159-199, fp32 as written there
int invert_transform(const float t[6], float inv[6])
{
    const volatile float bd = t[1] * t[3], ae = t[0] * t[4];
    const float eps = bd - ae;
    if (eps < 1e-8f && -eps < 1e-8f) return fail(NL_ERR_INVALID_ARG, "Matrix has no inverse, epsilon=%g", eps);
    const volatile float den1 = bd - ae, den2 = ae - bd;
    const volatile float ce = t[2] * t[4], bf = t[1] * t[5], cd = t[2] * t[3], af = t[0] * t[5];
    const volatile float n1 = ce - bf, n2 = cd - af;
    inv[0] = -t[4] / den1;
    inv[1] = t[1] / den1;
    inv[2] = n1 / den1;
    inv[3] = -t[3] / den2;
    inv[4] = t[0] / den2;
    inv[5] = n2 / den2;
    return NL_OK;
}

}  // namespace nl

extern "C" {

const char *nl_last_error(void) { return g_err.c_str(); }

const char *nl_version(void) { return "nlstack 0.2.0 (gfx950)"; }

void nl_release_cached_memory(void) { cache_release_all(); stream_pool_release_all(); pinned_release_all(); }

int nl_device_count(void)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(NL_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

static int destroy_impl(nl_stack_t *h)
{
    if (!h) return NL_OK;
    if (!h->stream) {             // create failed before anything existed on a device (e.g. a bad ordinal):
        delete h;                 // no HIP call, so no stale error is left behind for hipGetLastError
        return NL_OK;
    }
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->side_stream) (void)hipStreamSynchronize(h->side_stream);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    // (the large create-time buffers are parked for the next handle of the same geometry, see cached_free)
    cached_free(h->d_frames_owned, (size_t)h->fstride_owned * sizeof(float) * (size_t)h->n_capacity, h->device);
    cached_free(h->d_out, (size_t)h->npix * sizeof(float), h->device);
    if (h->d_acc) (void)hipFree(h->d_acc);
    if (h->d_reject_map) (void)hipFree(h->d_reject_map);
    if (h->d_coverage) (void)hipFree(h->d_coverage);
    if (h->ev_cov0) (void)hipEventDestroy(h->ev_cov0);
    if (h->ev_cov1) (void)hipEventDestroy(h->ev_cov1);
    if (h->d_weights) (void)hipFree(h->d_weights);
    if (h->d_xstat) (void)hipFree(h->d_xstat);
    if (h->d_sets) (void)hipFree(h->d_sets);
    cached_free(h->d_bounds, (size_t)nl::kBoundRounds * (size_t)h->npix * sizeof(float2), h->device);
    cached_free(h->d_nrounds, (size_t)h->npix, h->device);
    cached_free(h->d_fb_list, sizeof(unsigned) * (size_t)h->npix, h->device);
    cached_free(h->d_gen_list, sizeof(unsigned) * (size_t)h->npix, h->device);
    if (h->d_counters_own) (void)hipFree(h->d_counters_own);
    if (h->d_stat_partial) (void)hipFree(h->d_stat_partial);
    h->ingest.release();
    h->ingest_async.release();
    if (h->d_stat_partial_async) (void)hipFree(h->d_stat_partial_async);
    for (int i = 0; i < 2; i++) {          // (parked like the create-time buffers: a handle per Apply pays no hipMalloc for them)
        cached_free(h->d_lf_list[i], sizeof(unsigned) * (size_t)h->npix, h->device);
        cached_free(h->d_lf_state[i], sizeof(uint4) * (size_t)h->npix * (size_t)h->lf_lanes, h->device);
    }
    if (h->d_lf_count) (void)hipFree(h->d_lf_count);
    h->frame_scratch.release(h->device);
    for (int i = 0; i < kStageSlots; i++) {
        pinned_free(h->h_stage[i], h->stage_cap[i]);
        if (h->stage_done[i]) (void)hipEventDestroy(h->stage_done[i]);
    }
    park_copy_stream(h->copy_stream, h->device);
    for (int i = 0; i < kTimingRing; i++) {
        if (h->ring_start[i]) (void)hipEventDestroy(h->ring_start[i]);
        if (h->ring_stop[i]) (void)hipEventDestroy(h->ring_stop[i]);
        if (h->ring_dom0[i]) (void)hipEventDestroy(h->ring_dom0[i]);
        if (h->ring_dom1[i]) (void)hipEventDestroy(h->ring_dom1[i]);
    }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join) (void)hipEventDestroy(h->ev_join);
    for (hipEvent_t &ev : h->ev_order) if (ev) (void)hipEventDestroy(ev);
    park_stream_pair(h->stream, h->side_stream, h->device);
    delete h;
    return NL_OK;
}

void nl_stack_destroy(nl_stack_t *h) { destroy_impl(h); }

static int create_impl(nl_stack_t *h)
{
    const int rc = select_device(h->device);
    if (rc != NL_OK) return rc;
    // (main and side stream as the pair they were created as: different hardware queues, see the stream pool)
    NL_HIP(pooled_stream_pair(&h->stream, &h->side_stream, h->device));
    // (the timing events of a ring slot are created by the first pass that uses it: a handle that lives for ONE
    // Apply -- the cgo drop-in -- creates 4 events instead of 256)
    {
        // Events that only order device work against device work (fork / join of the side stream) or only take times: no
        // system-scope fence when they complete (hipEventDisableSystemFence) -- the writeback / invalidate it stands for costs
        // the next kernel 4 - 9 us per pass (512-row tile: 0.268 -> 0.259 ms, 32 frames 0.106 -> 0.099).  What the HOST reads
        // (counters, results) is ordered by the stream synchronisation of nl_stack_finish, not by these events.
        // NL_EV_FENCE=1 (developer switch): default events, for A/B runs.
        static const unsigned nofence = [] { const char *e = getenv("NL_EV_FENCE"); return e && e[0] == '1' ? 0u : (unsigned)hipEventDisableSystemFence; }();
        NL_HIP(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming | nofence));
        NL_HIP(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming | nofence));
        h->ev_rel = nofence;
    }
    const size_t frame_bytes = (size_t)h->npix * sizeof(float);
    h->fstride = h->fstride_owned = padded_frame_stride(h->npix);
    NL_HIP(cached_malloc((void **)&h->d_frames_owned, (size_t)h->fstride * sizeof(float) * (size_t)h->n_frames, h->device));
    h->d_frames = h->d_frames_owned;
    NL_HIP(cached_malloc((void **)&h->d_out, frame_bytes, h->device));
    NL_HIP(dev_malloc(&h->d_weights, sizeof(float) * (size_t)h->n_frames));
    h->max_grid = 256 * 64;
    NL_HIP(dev_malloc(&h->d_sets, 2 * kScratchBytes));
    NL_HIP(hipMemsetAsync(h->d_sets, 0, 2 * kScratchBytes, h->stream));
    h->cur_set = 0;
    h->d_partial = h->d_sets;
    h->d_fb_count = reinterpret_cast<unsigned *>(h->d_partial + 2 * nl::kClipSlots);
    if (h->npix < (int64_t)0xFFFFFFFFll) {
        NL_HIP(cached_malloc((void **)&h->d_fb_list, sizeof(unsigned) * (size_t)h->npix, h->device));
        NL_HIP(cached_malloc((void **)&h->d_gen_list, sizeof(unsigned) * (size_t)h->npix, h->device));
    }
    NL_HIP(dev_malloc(&h->d_counters_own, sizeof(unsigned long long) * 4));      // {clip_low, clip_high, list lengths (fused passes), -}
    h->d_counters = h->d_counters_own;
    NL_HIP(hipMemsetAsync(h->d_counters, 0, sizeof(unsigned long long) * 4, h->stream));
    NL_HIP(dev_malloc(&h->d_stat_partial, sizeof(double) * 3 * kStatBlocks));

    const std::vector<float> xstat = xstat_table(h->n_frames);
    NL_HIP(dev_malloc(&h->d_xstat, xstat.size() * sizeof(float)));
    NL_HIP(hipMemcpy(h->d_xstat, xstat.data(), xstat.size() * sizeof(float), hipMemcpyHostToDevice));
    return NL_OK;
}

nl_stack_t *nl_stack_create(int n_frames, int width, int height, int row0, int rows, int device)
{
    if (n_frames <= 0) { fail(NL_ERR_NO_INPUTS, "stack operator needs inputs"); return nullptr; }
    if (width <= 0 || height <= 0 || row0 < 0 || rows <= 0 || row0 + rows > height) {
        fail(NL_ERR_INVALID_ARG, "bad geometry %dx%d rows [%d,%d)", width, height, row0, row0 + rows);
        return nullptr;
    }
    nl_stack_t *h = new nl_stack();
    h->device = device; h->n_frames = h->n_capacity = n_frames; h->width = width; h->height = height;
    h->row0 = row0; h->rows = rows; h->npix = (int64_t)rows * width;
    if (create_impl(h) != NL_OK) {
        std::string keep = g_err;
        destroy_impl(h);
        g_err = keep;
        return nullptr;
    }
    return h;
}

int nl_stack_upload_frame(nl_stack_t *h, int idx, const float *host_frame)
{
    NL_CHECK_HANDLE(h);
    if (idx < 0 || idx >= h->n_frames || !host_frame)
        return fail(NL_ERR_INVALID_ARG, "upload_frame: bad index %d or null frame", idx);
    return nl_stack_upload_tile(h, idx, host_frame + (int64_t)h->row0 * h->width);
}

int nl_stack_upload_tile(nl_stack_t *h, int idx, const float *host_tile)
{
    NL_CHECK_HANDLE(h);
    if (idx < 0 || idx >= h->n_frames || !host_tile)
        return fail(NL_ERR_INVALID_ARG, "upload_tile: bad index %d or null tile", idx);
    NL_HIP(hipMemcpyAsync(h->d_frames + (int64_t)idx * h->fstride, host_tile,
                          (size_t)h->npix * sizeof(float), hipMemcpyHostToDevice, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));   // pointer must not be retained (cgo rules)
    return NL_OK;
}

// Overlapped uploads (the caller side of the path): `bytes` of host memory are copied by a few host
// threads into a pinned staging slot (ring of kStageSlots; a slot is re-used once its last DMA has left it) and the call
// returns (the caller's pointer is not retained, cgo rules); the DMA runs on the copy stream while the caller prepares the
// next frame, ordered behind the last pass that may still read the frames, and the next pass waits for it on the device.
// *staged = the pinned copy, *slot_out = its slot (record stage_done on the copy stream after the last operation that reads it).
static int stage_host_bytes(nl_stack_t *h, const void *src_v, size_t bytes, char **staged, int *slot_out)
{
    if (!h->copy_stream) NL_HIP(pooled_copy_stream(&h->copy_stream, h->device));
    if (h->pass_seq > 0 && h->copy_waits_pass != h->pass_seq) {
        // a pass enqueued earlier may still be reading the frames: the copy stream waits for its
        // end on the device (staging batch b+1 while batch b is stacked must not overwrite b)
        NL_HIP(hipStreamWaitEvent(h->copy_stream, h->ev_stop, 0));
        h->copy_waits_pass = h->pass_seq;
    }
    const int slot = h->stage_next;
    h->stage_next = (slot + 1) % kStageSlots;
    if (h->stage_used[slot]) NL_HIP(hipEventSynchronize(h->stage_done[slot]));     // its last DMA has left the buffer
    if (!h->stage_done[slot]) NL_HIP(hipEventCreateWithFlags(&h->stage_done[slot], hipEventDisableTiming));
    if (h->stage_cap[slot] < bytes) {
        if (h->h_stage[slot]) { pinned_free(h->h_stage[slot], h->stage_cap[slot]); h->h_stage[slot] = nullptr; h->stage_cap[slot] = 0; }
        NL_HIP(pinned_malloc(&h->h_stage[slot], bytes, &h->stage_cap[slot]));
    }
    const char *src = static_cast<const char *>(src_v);
    char *dst = static_cast<char *>(h->h_stage[slot]);
    if (bytes < ((size_t)4 << 20)) {
        memcpy(dst, src, bytes);
    } else {
        std::thread workers[kStageThreads - 1];
        const size_t part = (bytes / kStageThreads + 63) & ~(size_t)63;
        for (int t = 1; t < kStageThreads; t++) {
            const size_t b = (size_t)t * part, e = (b + part < bytes) ? b + part : bytes;
            workers[t - 1] = std::thread([=] { if (b < e) memcpy(dst + b, src + b, e - b); });
        }
        memcpy(dst, src, part < bytes ? part : bytes);
        for (auto &w : workers) w.join();
    }
    *staged = dst;
    *slot_out = slot;
    return NL_OK;
}

static int stage_done(nl_stack_t *h, int slot)
{
    NL_HIP(hipEventRecord(h->stage_done[slot], h->copy_stream));
    h->stage_used[slot] = true;
    h->uploads_pending = true;
    return NL_OK;
}

int nl_stack_upload_frame_async(nl_stack_t *h, int idx, const float *host_frame)
{
    NL_CHECK_HANDLE(h);
    if (idx < 0 || idx >= h->n_frames || !host_frame)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_async: bad index %d or null frame", idx);
    if (h->d_frames != h->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_async: frames are attached, not owned");
    const size_t bytes = (size_t)h->npix * sizeof(float);
    char *dst = nullptr;
    int slot = 0;
    int rc = stage_host_bytes(h, host_frame + (int64_t)h->row0 * h->width, bytes, &dst, &slot);
    if (rc != NL_OK) return rc;
    // (fp32 frames keep the copy engine: a kernel that pulls the frame out of the pinned buffer itself, as the FITS decode
    // below does, measured 41.6 against 43.3 GiB/s on the same box -- profiles/r06_apply_from_host.txt)
    NL_HIP(hipMemcpyAsync(h->d_frames + (int64_t)idx * h->fstride, dst, bytes, hipMemcpyHostToDevice, h->copy_stream));
    return stage_done(h, slot);
}

// Host-side wait for every asynchronous upload issued so far.
int nl_stack_upload_wait(nl_stack_t *h)
{
    NL_CHECK_HANDLE(h);
    if (h->copy_stream) NL_HIP(hipStreamSynchronize(h->copy_stream));
    h->uploads_pending = false;
    return NL_OK;
}

int nl_stack_download_tile(nl_stack_t *h, int idx, float *host_tile)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    if (idx < 0 || idx >= h->n_frames || !host_tile)
        return fail(NL_ERR_INVALID_ARG, "download_tile: bad index %d or null tile", idx);
    NL_HIP(hipMemcpyAsync(host_tile, h->d_frames + (int64_t)idx * h->fstride,
                          (size_t)h->npix * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl_stack_download_rows(nl_stack_t *h, int idx, int first_row, int n_rows, float *host_rows)
{
    NL_CHECK_HANDLE(h);
    NL_SETTLE_UPLOADS(h);
    if (idx < -1 || idx >= h->n_frames || !host_rows || first_row < 0 || n_rows <= 0 ||
        (int64_t)first_row + n_rows > h->rows)
        return fail(NL_ERR_INVALID_ARG, "download_rows: bad index %d, rows [%d,%d) of %d, or null buffer",
                    idx, first_row, first_row + n_rows, h->rows);
    const float *src = (idx < 0 ? h->d_out : h->d_frames + (int64_t)idx * h->fstride) + (int64_t)first_row * h->width;
    NL_HIP(hipMemcpyAsync(host_rows, src, (size_t)n_rows * h->width * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// Device memory the handle holds right now: the buffers of nl_stack_create plus everything a pass, an upload path or
// the stack of stacks has allocated since (decision-pass thresholds, linear-fit cascade lists, accumulator, ingest
// staging, the scratch of the steps on one frame) -- those stay until nl_stack_destroy, so a caller that sizes batches
// to the device (OpStackBatches, stackbatches.go:121-187 does it for host memory) can see what is left.
int64_t nl_stack_device_bytes(nl_stack_t *h)
{
    if (!h) return 0;
    const int64_t np = h->npix;
    int64_t b = 0;
    if (h->d_frames_owned) b += h->fstride_owned * 4 * h->n_capacity;
    if (h->d_out) b += np * 4;
    if (h->d_acc) b += np * 4;
    if (h->d_reject_map) b += np * 4;
    if (h->d_coverage) b += np * 2;
    if (h->d_weights) b += 4 * (int64_t)h->n_capacity;
    if (h->d_xstat) b += 8 * (int64_t)(h->n_capacity + 1);
    if (h->d_sets) b += 2 * (int64_t)kScratchBytes;
    if (h->d_bounds) b += (int64_t)nl::kBoundRounds * np * 8;
    if (h->d_nrounds) b += np;
    if (h->d_fb_list) b += np * 4;
    if (h->d_gen_list) b += np * 4;
    if (h->d_counters) b += 32;
    if (h->d_stat_partial) b += 8 * 3 * kStatBlocks;
    if (h->d_stat_partial_async) b += 8 * 3 * kStatBlocks;
    const int lanes = h->n_capacity <= 128 ? 1 : h->n_capacity <= 256 ? 2 : 4;
    for (int i = 0; i < 2; i++) {
        if (h->d_lf_list[i]) b += np * 4;
        if (h->d_lf_state[i]) b += np * 16 * lanes;
    }
    if (h->d_lf_count) b += 4 * nl::kLinfitCounters;
    b += (int64_t)h->ingest.bytes + (int64_t)h->ingest_async.bytes + (int64_t)h->frame_scratch.bytes();
    return b;
}

void *nl_stack_frames_device_ptr(nl_stack_t *h) { return h ? h->d_frames : nullptr; }
void *nl_stack_result_device_ptr(nl_stack_t *h) { return h ? h->d_out : nullptr; }
int nl_stack_last_mode(nl_stack_t *h) { return h ? h->last_mode : -1; }
const char *nl_stack_last_kernel_name(nl_stack_t *h) { return h ? h->last_kernel : ""; }

int nl_stack_attach_device_frames_strided(nl_stack_t *h, void *device_frames, int64_t frame_stride)
{
    NL_CHECK_HANDLE(h);
    if (!device_frames) {
        h->d_frames = h->d_frames_owned;
        h->fstride = h->fstride_owned;
        return NL_OK;
    }
    // the kernels address 4 frames + a pixel with one signed 32-bit byte offset (fast_common.hpp gather_sorted,
    // fast_ml_common.hpp ml_gather_raw) and load 16 bytes per lane where the stride allows; the owned buffer's stride
    // is chosen inside these limits, a lent one is checked
    if (frame_stride < h->npix)
        return fail(NL_ERR_INVALID_ARG, "attach_device_frames: stride %lld < %lld pixels of the tile",
                    (long long)frame_stride, (long long)h->npix);
    if (h->npix < nl::kFastMaxPixels && !frame_stride_addressable(h->npix, frame_stride))
        return fail(NL_ERR_INVALID_ARG, "attach_device_frames: stride %lld too large for the tile's 32-bit frame offsets",
                    (long long)frame_stride);
    h->d_frames = static_cast<float *>(device_frames);
    h->fstride = frame_stride;
    return NL_OK;
}

int nl_stack_attach_device_frames(nl_stack_t *h, void *device_frames)
{
    NL_CHECK_HANDLE(h);
    return nl_stack_attach_device_frames_strided(h, device_frames, h->npix);
}

int64_t nl_stack_frame_stride(nl_stack_t *h)
{
    return h ? h->fstride : 0;
}

int nl_stack_fill_synthetic(nl_stack_t *h, uint64_t seed)
{
    NL_CHECK_HANDLE(h);
    NL_HIP(nl::launch_fill_synthetic(h->d_frames, h->fstride, h->n_frames, h->width, h->height,
                                     h->row0, h->rows, seed, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// Frames in use for the next passes: slots [0, n) of the n_capacity allocated at create.  The
// caller of a batch loop (OpStackBatches, stackbatches.go:69-111) keeps ONE handle -- buffers,
// accumulator -- across batches whose last one is smaller.
int nl_stack_set_active_frames(nl_stack_t *h, int n)
{
    NL_CHECK_HANDLE(h);
    if (n < 1 || n > h->n_capacity)
        return fail(NL_ERR_INVALID_ARG, "set_active_frames: %d not in [1, %d]", n, h->n_capacity);
    if (n != h->n_frames) h->has_weights = false;      // weights are per frame of a given batch
    h->n_frames = n;
    return NL_OK;
}

int nl_stack_set_weights(nl_stack_t *h, const float *weights)
{
    NL_CHECK_HANDLE(h);
    if (!weights) { h->has_weights = false; return NL_OK; }
    NL_HIP(hipMemcpyAsync(h->d_weights, weights, sizeof(float) * (size_t)h->n_frames,
                          hipMemcpyHostToDevice, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    h->has_weights = true;
    return NL_OK;
}

// getWeights, stack.go:231-270 (scalar host arithmetic, fp32, same order)
int nl_weights_from_scalars(int weighting, const float *per_frame, int n_frames,
                            float *weights_out, int *bad_index)
{
    if (bad_index) *bad_index = -1;
    if (weighting == NL_WEIGHT_NONE) return NL_OK;
    if (!per_frame || !weights_out || n_frames <= 0)
        return fail(NL_ERR_INVALID_ARG, "weights_from_scalars: null argument");
    if (weighting == NL_WEIGHT_EXPOSURE) {
        for (int i = 0; i < n_frames; i++) {
            if (per_frame[i] == 0) {
                if (bad_index) *bad_index = i;
                return fail(NL_ERR_MISSING_EXPOSURE,
                            "%d: Missing exposure information for exposure-weighted stacking", i);
            }
            weights_out[i] = per_frame[i];
        }
        return NL_OK;
    }
    if (weighting == NL_WEIGHT_INVERSE_NOISE || weighting == NL_WEIGHT_INVERSE_HFR) {
        float mn = 3.40282346638528859811704183484516925440e+38f, mx = -mn;
        for (int i = 0; i < n_frames; i++) {
            const float v = per_frame[i];
            if (v < mn) mn = v;
            if (v > mx) mx = v;
        }
        const float range = mx - mn;
        for (int i = 0; i < n_frames; i++) {
            volatile float num = per_frame[i] - mn;
            num = 4.0f * num;
            volatile float q = num / range;
            volatile float den = 1.0f + q;
            weights_out[i] = 1.0f / den;
        }
        return NL_OK;
    }
    return fail(NL_ERR_INVALID_WEIGHTING, "Invalid weighting mode %d\n", weighting);
}

// ---- formats and steps either side of the stack (ingest.hip) ----------------------
// min / max / mean from the decode kernel's per-block partials (read.go:210: mean = float32(sum/len))
static int decode_stats(nl_stack_t *h, int64_t n, float *stats_out)
{
    std::vector<double> part(3 * kStatBlocks);
    NL_HIP(hipMemcpyAsync(part.data(), h->d_stat_partial, sizeof(double) * 3 * kStatBlocks,
                          hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    float lo = (float)part[0], hi = (float)part[1];
    double sum = 0.0;
    for (int b = 0; b < kStatBlocks; b++) {
        const float bl = (float)part[3 * b], bh = (float)part[3 * b + 1];
        if (bl < lo) lo = bl;
        if (bh > hi) hi = bh;
        sum += part[3 * b + 2];
    }
    stats_out[0] = lo;
    stats_out[1] = hi;
    stats_out[2] = (float)(sum / (double)n);
    return NL_OK;
}

// the argument checks of both FITS uploads; *bytes = the payload's size
static int fits_upload_check(nl_stack_t *h, int idx, const void *raw_host, int bitpix, size_t *bytes)
{
    if (idx < 0 || idx >= h->n_frames || !raw_host)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_fits: bad index %d or null payload", idx);
    const int bpv = nl::fits_bytes_per_value(bitpix);
    if (bpv == 0) return fail(NL_ERR_INVALID_ARG, "Unknown BITPIX value %d", bitpix);      // read.go:169
    if (h->d_frames != h->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_fits: frames are attached, not owned");
    *bytes = (size_t)h->npix * (size_t)bpv;
    return NL_OK;
}

// the argument checks of both projected uploads; inv = the inverse transform, *bytes = the source frame's size
static int projected_upload_check(nl_stack_t *h, int idx, const float *src_host, int src_w, int src_h,
                                  const float trans[6], float inv[6], size_t *bytes)
{
    if (idx < 0 || idx >= h->n_frames || !src_host || !trans || src_w < 1 || src_h < 1)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_projected: bad argument (frame %d)", idx);
    if (h->d_frames != h->d_frames_owned)
        return fail(NL_ERR_INVALID_ARG, "upload_frame_projected: frames are attached, not owned");
    *bytes = (size_t)src_w * (size_t)src_h * sizeof(float);
    return invert_transform(trans, inv);
}

int nl_stack_upload_frame_fits(nl_stack_t *h, int idx, const void *raw_host, int bitpix, float bscale,
                               float bzero, float multiplier, float offset, float *stats_out)
{
    NL_CHECK_HANDLE(h);
    size_t bytes = 0;
    int rc = fits_upload_check(h, idx, raw_host, bitpix, &bytes);
    if (rc != NL_OK) return rc;
    NL_HIP(h->ingest.reserve(bytes, h->stream));
    NL_HIP(hipMemcpyAsync(h->ingest.ptr, raw_host, bytes, hipMemcpyHostToDevice, h->stream));
    const bool affine = !(multiplier == 1.0f && offset == 0.0f);
    NL_HIP(nl::launch_fits_decode(h->ingest.ptr, bitpix, h->npix, bscale, bzero, affine, multiplier, offset,
                                  h->d_frames + (int64_t)idx * h->fstride, h->d_stat_partial, kStatBlocks,
                                  h->stream));
    if (stats_out) return decode_stats(h, h->npix, stats_out);
    NL_HIP(hipStreamSynchronize(h->stream));          // the caller's buffer must not be read after return
    return NL_OK;
}

int nl_stack_upload_frame_projected(nl_stack_t *h, int idx, const float *src_host, int src_w, int src_h,
                                    const float trans[6], float out_of_bounds, float multiplier, float offset)
{
    NL_CHECK_HANDLE(h);
    float inv[6];
    size_t bytes = 0;
    int rc = projected_upload_check(h, idx, src_host, src_w, src_h, trans, inv, &bytes);
    if (rc != NL_OK) return rc;
    NL_HIP(h->ingest.reserve(bytes, h->stream));
    NL_HIP(hipMemcpyAsync(h->ingest.ptr, src_host, bytes, hipMemcpyHostToDevice, h->stream));
    const bool affine = !(multiplier == 1.0f && offset == 0.0f);
    NL_HIP(nl::launch_project(static_cast<const float *>(h->ingest.ptr), src_w, src_h,
                              h->d_frames + (int64_t)idx * h->fstride, h->width, h->row0, h->rows, inv,
                              out_of_bounds, affine, multiplier, offset, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// device scratch of the overlapped ingest (copy stream: operations on it are stream-ordered, one buffer serves
// every frame in flight)
static int ingest_async_reserve(nl_stack_t *h, size_t bytes)
{
    if (!h->d_stat_partial_async) NL_HIP(dev_malloc(&h->d_stat_partial_async, sizeof(double) * 3 * kStatBlocks));
    NL_HIP(h->ingest_async.reserve(bytes, h->copy_stream));
    return NL_OK;
}

int nl_stack_upload_frame_fits_async(nl_stack_t *h, int idx, const void *raw_host, int bitpix, float bscale,
                                     float bzero, float multiplier, float offset)
{
    NL_CHECK_HANDLE(h);
    size_t bytes = 0;
    int rc = fits_upload_check(h, idx, raw_host, bitpix, &bytes);
    if (rc != NL_OK) return rc;
    char *staged = nullptr;
    int slot = 0;
    rc = stage_host_bytes(h, raw_host, bytes, &staged, &slot);
    if (rc != NL_OK) return rc;
    // The decode kernel reads the payload straight out of the pinned staging buffer (round 6): DMA into a device scratch
    // and a kernel behind it on one stream took turns -- copy engine, compute queue, copy engine ... with a dependency
    // hand-over each way -- and ran at 0.9 ms per 32 MiB int16 frame where the link needs 0.6 (bench.py apply_from_host:
    // 34.7 GiB/s).  One kernel per frame that pulls its bytes over the link itself (8- or 16-byte loads per lane) has no hand-over at all.
    // NL_FITS_ZEROCOPY=0: the DMA + kernel pair, for A/B runs.
    static const bool zero_copy = [] { const char *e = getenv("NL_FITS_ZEROCOPY"); return !e || atoi(e) != 0; }();
    const void *raw_dev = staged;
    if (!zero_copy) {
        rc = ingest_async_reserve(h, bytes);
        if (rc != NL_OK) return rc;
        NL_HIP(hipMemcpyAsync(h->ingest_async.ptr, staged, bytes, hipMemcpyHostToDevice, h->copy_stream));
        raw_dev = h->ingest_async.ptr;
    } else if (!h->d_stat_partial_async) {
        NL_HIP(dev_malloc(&h->d_stat_partial_async, sizeof(double) * 3 * kStatBlocks));
    }
    const bool affine = !(multiplier == 1.0f && offset == 0.0f);
    NL_HIP(nl::launch_fits_decode(raw_dev, bitpix, h->npix, bscale, bzero, affine, multiplier, offset,
                                  h->d_frames + (int64_t)idx * h->fstride, h->d_stat_partial_async, kStatBlocks,
                                  h->copy_stream));
    return stage_done(h, slot);
}

int nl_stack_upload_frame_projected_async(nl_stack_t *h, int idx, const float *src_host, int src_w, int src_h,
                                          const float trans[6], float out_of_bounds, float multiplier, float offset)
{
    NL_CHECK_HANDLE(h);
    float inv[6];
    size_t bytes = 0;
    int rc = projected_upload_check(h, idx, src_host, src_w, src_h, trans, inv, &bytes);
    if (rc != NL_OK) return rc;
    char *staged = nullptr;
    int slot = 0;
    rc = stage_host_bytes(h, src_host, bytes, &staged, &slot);
    if (rc != NL_OK) return rc;
    rc = ingest_async_reserve(h, bytes);
    if (rc != NL_OK) return rc;
    NL_HIP(hipMemcpyAsync(h->ingest_async.ptr, staged, bytes, hipMemcpyHostToDevice, h->copy_stream));
    const bool affine = !(multiplier == 1.0f && offset == 0.0f);
    NL_HIP(nl::launch_project(static_cast<const float *>(h->ingest_async.ptr), src_w, src_h,
                              h->d_frames + (int64_t)idx * h->fstride, h->width, h->row0, h->rows, inv,
                              out_of_bounds, affine, multiplier, offset, h->copy_stream));
    return stage_done(h, slot);
}

int nl_stack_download_result_fits(nl_stack_t *h, void *raw_host)
{
    NL_CHECK_HANDLE(h);
    if (!raw_host) return fail(NL_ERR_INVALID_ARG, "download_result_fits: null buffer");
    if (h->pending) return fail(NL_ERR_INVALID_ARG, "download_result_fits: a pass is still pending (call nl_stack_finish)");
    const size_t bytes = (size_t)h->npix * sizeof(float);
    NL_HIP(h->ingest.reserve(bytes, h->stream));
    NL_HIP(nl::launch_fits_encode(h->d_out, h->npix, 1, h->ingest.ptr, h->stream));
    NL_HIP(hipMemcpyAsync(raw_host, h->ingest.ptr, bytes, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

int nl_fits_decode(const void *raw_host, int bitpix, int64_t n, float bscale, float bzero, float *out_host,
                   float *stats_out, int device)
{
    if (!raw_host || !out_host || n < 1 || n > 0x7fffffff)
        return fail(NL_ERR_INVALID_ARG, "fits_decode: bad argument");
    if (nl::fits_bytes_per_value(bitpix) == 0) return fail(NL_ERR_INVALID_ARG, "Unknown BITPIX value %d", bitpix);
    // (a handle of n x 1 pixels)
    return with_scratch_handle((int)n, 1, device, [&](nl_stack_t *h) {
        int rc = nl_stack_upload_frame_fits(h, 0, raw_host, bitpix, bscale, bzero, 1.0f, 0.0f, stats_out);
        return rc == NL_OK ? nl_stack_download_tile(h, 0, out_host) : rc;
    });
}

int nl_project_bilinear(const float *src_host, int src_w, int src_h, float *dst_host, int dst_w, int dst_h,
                        const float trans[6], float out_of_bounds, int device)
{
    if (!src_host || !dst_host || dst_w < 1 || dst_h < 1)
        return fail(NL_ERR_INVALID_ARG, "project_bilinear: bad argument");
    return with_scratch_handle(dst_w, dst_h, device, [&](nl_stack_t *h) {
        int rc = nl_stack_upload_frame_projected(h, 0, src_host, src_w, src_h, trans, out_of_bounds, 1.0f, 0.0f);
        return rc == NL_OK ? nl_stack_download_tile(h, 0, dst_host) : rc;
    });
}

}  // extern "C"
