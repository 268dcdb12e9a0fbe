// locscale.hip -- Stats.Location() / Scale() of one resident frame for gfx950 (internal/stats/stats.go:225-244),
// bit-exact given the seeds.
//
// The reference's sampling functions each start a fresh fastrand.RNG: xorshift32 from a seed the caller now passes.
// One call of them is, all on one stream:
//   locscale_draws           the raw draws of one round.  xorshift32 is linear over GF(2): one lane per chunk of 64
//                            draws jumps from the round's start state to its chunk's by the binary powers of the
//                            64-step matrix (kernel argument), then steps 64 times.  The last draw is the state the
//                            next round starts from.
//   locscale_gather          unbounded calls: one lane per sample, index by the 32 x 32 -> high 32 multiply, pixel load
//   locscale_gather_bounded  bounded calls: one lane per draw position; the median's pixel and accept flag, or for Qn
//                            both roles of the position (first draw of a pair; second draw of the pair the position
//                            before it opened) with their flags
//   locscale_compact         one workgroup: which positions emit a sample (Qn: the automaton of :455-465, below), an
//                            ordered prefix sum, ranks < num_samples kept, the position of the last one = draws consumed
//   locscale_select          the radix select of select_common.hpp over the samples in global memory, one workgroup
//                            per rank (two for the median of an even count), and the NaN count
// then one read-back of the call state.  The loop of :477-499 and the arithmetic on the selected values run on the
// host.  LSEHistogram: locscale_hist (per-workgroup LDS bins, merged with global atomics), peak and cumulation on the
// host from the 4096 counts.
//
// The automaton of FastApproxBoundedQn: a position is a pair's second draw iff the position before it was a first
// draw that was accepted; after a second draw comes a first draw whatever happened.  By induction a position is a
// second draw iff the run of accepted-as-first positions that ends right before it has odd length, so the states
// follow from the last position whose first-draw test failed: a running maximum instead of a scan over 2-to-2 maps.
#include <math.h>

#include <algorithm>
#include <vector>

#include "frame_common.hpp"
#include "launch_common.hpp"
#include "locscale.hpp"
#include "select_common.hpp"

namespace nl {

namespace {

constexpr int kChunk = 64;             // draws one lane of locscale_draws steps through
constexpr int kJumpLevels = 16;        // chunks of one round < 2^16 (kLocScaleMaxSamples)
constexpr int kCompactThreads = 1024;
constexpr int kCompactPer = 4;         // positions per lane and tile of locscale_compact
constexpr int kCompactTile = kCompactThreads * kCompactPer;
constexpr int kHistThreads = 256;
constexpr int kHistBlocks = 1024;

enum { kMedian = 0, kMad = 1, kQn = 2 };

// col[l][b]: the state 64 * 2^l steps after the state 1 << b
struct JumpTable {
    uint32_t col[kJumpLevels][32];
};

// the state of one sampling call on the device, read back once per round
struct CallState {
    uint32_t rng[2];                   // the state a round starts from / leaves, alternating
    uint32_t filled;                   // samples emitted so far (may pass num_samples)
    uint32_t consumed;                 // bounded: draws up to and including the one that filled the samples
    uint32_t run_start;                // bounded Qn: the position behind the last failed first-draw test
    uint32_t nan;                      // NaNs among the samples
    float sel[2];                      // the selected ranks
};

__host__ __device__ inline uint32_t xorshift32(uint32_t x)
{
    x ^= x << 13;
    x ^= x >> 17;
    x ^= x << 5;
    return x;
}

__host__ __device__ inline uint32_t jump(const uint32_t *col, uint32_t x)
{
    uint32_t y = 0;
    for (int b = 0; b < 32; b++) y ^= ((x >> b) & 1u) ? col[b] : 0u;
    return y;
}

const JumpTable &jump_table()
{
    static const JumpTable table = [] {
        JumpTable t;
        for (int b = 0; b < 32; b++) {
            uint32_t x = 1u << b;
            for (int s = 0; s < kChunk; s++) x = xorshift32(x);
            t.col[0][b] = x;
        }
        for (int l = 1; l < kJumpLevels; l++)
            for (int b = 0; b < 32; b++) t.col[l][b] = jump(t.col[l - 1], t.col[l - 1][b]);
        return t;
    }();
    return table;
}

// raw[0 .. 64 n_chunks): the draws behind the state `seed` (first) or st->rng[slot]; st->rng[slot ^ 1] = the last one
__global__ __launch_bounds__(256) void locscale_draws_kernel(JumpTable jt, uint32_t seed, int first, int slot,
                                                             int n_chunks, uint32_t *raw, CallState *st)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_chunks) return;
    uint32_t x = first ? seed : st->rng[slot];
    for (int l = 0; l < kJumpLevels; l++)
        if ((c >> l) & 1) x = jump(jt.col[l], x);
    uint32_t *out = raw + (size_t)c * kChunk;
    for (int j = 0; j < kChunk; j++) {
        x = xorshift32(x);
        out[j] = x;
    }
    if (c == n_chunks - 1) st->rng[slot ^ 1] = x;
}

// rng.Uint32n(m)
__device__ __forceinline__ uint32_t uint32n(uint32_t x, uint32_t m) { return __umulhi(x, m); }

// FastApproxMedian (:339-342), FastApproxMAD (:404-407), FastApproxQn (:439-443): sample i of n
template <int KIND>
__global__ __launch_bounds__(256) void locscale_gather_kernel(const float *data, uint32_t pixels, const uint32_t *raw,
                                                              int n, float location, float *samples)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (KIND == kQn) {
        const uint32_t i1 = 1u + uint32n(raw[2 * i], pixels - 1u);
        const uint32_t i2 = uint32n(raw[2 * i + 1], i1);
        samples[i] = fabsf(data[i1] - data[i2]);
    } else {
        const float d = data[uint32n(raw[i], pixels)];
        samples[i] = KIND == kMad ? fabsf(d - location) : d;
    }
}

// Position p of n of a bounded round.  Median (:355-356): val = the pixel, flag 1 = within [lo, hi].  Qn (:456-464):
// flag bit 0 = as a pair's first draw the position passes :458 (a NaN pixel does); bit 1 and val = as the second draw
// of the pair the position before opened (its raw draw: raw[p - 1], or the state the round started from) the pixel
// is within the bounds, and |d1 - d2|.
template <bool QN>
__global__ __launch_bounds__(256) void locscale_gather_bounded_kernel(const float *data, uint32_t pixels,
                                                                      const uint32_t *raw, int n, int first, int slot,
                                                                      const CallState *st, float lo, float hi,
                                                                      float *val, unsigned char *flags)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const uint32_t r = raw[p];
    if (!QN) {
        const float d = data[uint32n(r, pixels)];
        val[p] = d;
        flags[p] = (d >= lo && d <= hi) ? 1 : 0;
    } else {
        const float d1 = data[1u + uint32n(r, pixels - 1u)];
        const unsigned ok_first = (d1 < lo || d1 > hi) ? 0u : 1u;
        const uint32_t prev = p > 0 ? raw[p - 1] : (first ? 0u : st->rng[slot]);
        const uint32_t i1 = 1u + uint32n(prev, pixels - 1u);
        const float e1 = data[i1];
        const float d2 = data[uint32n(r, i1)];
        const unsigned ok_second = (d2 >= lo && d2 <= hi) ? 2u : 0u;
        val[p] = fabsf(e1 - d2);
        flags[p] = (unsigned char)(ok_first | ok_second);
    }
}

// inclusive scans over a wave of 64
__device__ __forceinline__ unsigned wave_scan_sum(unsigned v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_scan_max(unsigned v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned t = __shfl_up(v, d, 64);
        if (lane >= d) v = max(v, t);
    }
    return v;
}

// The samples of a bounded round, in stream order behind the st->filled there are: positions pos0 .. pos0 + n - 1 of
// the call's stream, val / flags as locscale_gather_bounded left them (both padded to whole tiles).  One workgroup.
template <bool QN>
__global__ __launch_bounds__(kCompactThreads) void locscale_compact_kernel(const float *val, const unsigned char *flags,
                                                                           int n, uint32_t pos0, uint32_t want,
                                                                           CallState *st, float *samples)
{
    __shared__ unsigned s_max[kCompactThreads / 64], s_sum[kCompactThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned base = st->filled, run_start = st->run_start;
    __syncthreads();                   // (thread 0 writes both at the end)
    for (int t0 = 0; t0 < n && base < want; t0 += kCompactTile) {
        const int i0 = t0 + (int)threadIdx.x * kCompactPer;
        const float4 v4 = *reinterpret_cast<const float4 *>(val + i0);
        const uint32_t f4 = *reinterpret_cast<const uint32_t *>(flags + i0);
        const float v[kCompactPer] = {v4.x, v4.y, v4.z, v4.w};
        unsigned f[kCompactPer];
        bool emit[kCompactPer];
#pragma unroll
        for (int j = 0; j < kCompactPer; j++) f[j] = i0 + j < n ? (f4 >> (8 * j)) & 255u : (QN ? 1u : 0u);
        if (QN) {
            // the position behind the last failed first-draw test in front of this lane's positions
            unsigned mine = 0;
#pragma unroll
            for (int j = 0; j < kCompactPer; j++)
                if (!(f[j] & 1u)) mine = pos0 + (unsigned)(i0 + j) + 1u;
            const unsigned incl = wave_scan_max(mine, lane);
            unsigned before = __shfl_up(incl, 1, 64);
            if (lane == 0) before = 0;
            if (lane == 63) s_max[wave] = incl;
            __syncthreads();
            unsigned all = 0;
            for (int w = 0; w < kCompactThreads / 64; w++) {
                if (w < wave) before = max(before, s_max[w]);
                all = max(all, s_max[w]);
            }
            unsigned m = max(run_start, before);
#pragma unroll
            for (int j = 0; j < kCompactPer; j++) {
                const unsigned g = pos0 + (unsigned)(i0 + j);
                emit[j] = i0 + j < n && ((g - m) & 1u) && (f[j] & 2u);
                if (!(f[j] & 1u)) m = g + 1u;
            }
            run_start = max(run_start, all);
        } else {
#pragma unroll
            for (int j = 0; j < kCompactPer; j++) emit[j] = f[j] != 0;
        }
        unsigned cnt = 0;
#pragma unroll
        for (int j = 0; j < kCompactPer; j++) cnt += emit[j] ? 1u : 0u;
        const unsigned incl = wave_scan_sum(cnt, lane);
        if (lane == 63) s_sum[wave] = incl;
        __syncthreads();
        unsigned rank = base + incl - cnt, total = 0;
        for (int w = 0; w < kCompactThreads / 64; w++) {
            if (w < wave) rank += s_sum[w];
            total += s_sum[w];
        }
#pragma unroll
        for (int j = 0; j < kCompactPer; j++) {
            if (!emit[j]) continue;
            if (rank < want) samples[rank] = v[j];
            if (rank + 1u == want) st->consumed = pos0 + (unsigned)(i0 + j) + 1u;
            rank++;
        }
        base += total;
        // the next tile's lane 63 writes s_sum (and s_max) again: not before every lane has read this tile's.  (The
        // Qn path had the barrier behind s_max in between; the median path had none.)
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        st->filled = base;
        st->run_start = run_start;
    }
}

// st->sel[blockIdx.x] = the sample of rank k0 + blockIdx.x (1-based) of n; block 0 also counts the NaNs
__global__ __launch_bounds__(kSelectThreads) void locscale_select_kernel(const float *samples, int n, unsigned k0,
                                                                         CallState *st)
{
    __shared__ SelectShared sh;
    if (blockIdx.x == 0) {
        unsigned nan = 0;
        for (int i = threadIdx.x; i < n; i += kSelectThreads) nan += samples[i] != samples[i] ? 1u : 0u;
        nan = block_sum(nan, sh.red);
        if (threadIdx.x == 0) st->nan = nan;
        __syncthreads();
    }
    const uint32_t key = block_select(n, k0 + blockIdx.x, [&](int i, uint32_t *out_key) {
        *out_key = f2key(samples[i]);
        return true;
    }, sh);
    if (threadIdx.x == 0) st->sel[blockIdx.x] = key2f(key);
}

// bins[uint32((d - min) * valueToBin + 0.5)]++ (:651-654); bins[kLocScaleBins]: the pixels whose bin the reference
// would index out of range (a NaN pixel, a stale min / max)
__global__ __launch_bounds__(kHistThreads) void locscale_hist_kernel(const float *data, int64_t n, float mn,
                                                                     float value_to_bin, uint32_t *bins)
{
    __shared__ unsigned h[kLocScaleBins];
    for (int b = threadIdx.x; b < kLocScaleBins; b += kHistThreads) h[b] = 0;
    __syncthreads();
    unsigned outside = 0;
    auto add = [&](float d) {
        const float t = (d - mn) * value_to_bin + 0.5f;     // truncation toward zero: (-1, 0) is bin 0
        if (t > -1.0f && t < (float)kLocScaleBins) atomicAdd(&h[(unsigned)(int)t], 1u);
        else outside++;
    };
    const int64_t quads = n >> 2;
    const float4 *d4 = reinterpret_cast<const float4 *>(data);
    for (int64_t q = (int64_t)blockIdx.x * kHistThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kHistThreads) {
        const float4 v = d4[q];
        add(v.x); add(v.y); add(v.z); add(v.w);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (int64_t i = quads << 2; i < n; i++) add(data[i]);
    __syncthreads();
    for (int b = threadIdx.x; b < kLocScaleBins; b += kHistThreads)
        if (h[b]) atomicAdd(&bins[b], h[b]);
    outside = wave_sum(outside);
    if ((threadIdx.x & 63) == 0 && outside) atomicAdd(&bins[kLocScaleBins], outside);
}

int invalid(std::string *msg, const std::string &m)
{
    *msg = m;
    return NL_ERR_INVALID_ARG;
}

int round_up(int64_t v, int to) { return (int)((v + to - 1) / to * to); }

// one frame, one estimate: the scratch carved, the sampling calls
struct Sampler {
    const float *data;
    uint32_t pixels;
    int want;                          // num_samples
    hipStream_t stream;
    std::string *msg;
    CallState *d_state = nullptr;
    uint32_t *d_raw = nullptr, *d_bins = nullptr;
    float *d_val = nullptr, *d_samples = nullptr;
    unsigned char *d_flags = nullptr;
    int round_median = 0, round_qn = 0;

    size_t carve(void *base)
    {
        round_median = round_up((int64_t)want + want / 4, kChunk);             // about 1.25 S
        round_qn = round_up(2 * (int64_t)want + want / 2, kChunk);             // about 2.5 S, and >= 2 S
        const size_t tile = (size_t)round_up(round_qn, kCompactTile);
        Carver c(base);
        d_state = c.take<CallState>(1);
        d_raw = c.take<uint32_t>((size_t)round_qn);
        d_val = c.take<float>(tile);
        d_flags = c.take<unsigned char>(tile);
        d_samples = c.take<float>((size_t)want);
        d_bins = c.take<uint32_t>(kLocScaleBins + 1);
        return align_up(c.bytes());
    }

    int read_state(CallState *s)
    {
        NL_RUN_HIP(hipMemcpyAsync(s, d_state, sizeof *s, hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipStreamSynchronize(stream));
        return NL_OK;
    }

    void draws(Launcher &L, uint32_t seed, bool first, int slot, int n)
    {
        const int chunks = (n + kChunk - 1) / kChunk;
        L(locscale_draws_kernel, (chunks + 255) / 256, 256, 0, jump_table(), seed, first ? 1 : 0, slot, chunks, d_raw,
          d_state);
    }

    // the median of the samples (QSelectMedianFloat32) or their first quartile (QSelectFirstQuartileFloat32)
    void select(Launcher &L, bool quartile)
    {
        const unsigned k = quartile ? (unsigned)(want >> 2) + 1u : (unsigned)(want >> 1) + 1u;
        const bool two = !quartile && !(want & 1);
        L(locscale_select_kernel, two ? 2 : 1, kSelectThreads, 0, d_samples, want, two ? k - 1u : k, d_state);
    }
    float selected(const CallState &s, bool quartile) const
    {
        return !quartile && !(want & 1) ? 0.5f * (s.sel[0] + s.sel[1]) : s.sel[0];
    }

    int nan_error(const char *fn, int call, unsigned count)
    {
        return invalid(msg, std::string(fn) + " (sampling call " + std::to_string(call) + "): " + std::to_string(count) +
                                " NaN among the samples; QSelectFloat32 (qsort.go:94-126) requires NaN-free input");
    }

    // FastApproxMedian / FastApproxMAD / FastApproxQn: the selected value before its normalisation
    int unbounded(int kind, int call, uint32_t seed, float location, float *out, uint32_t *consumed)
    {
        static const char *const names[3] = {"FastApproxMedian", "FastApproxMAD", "FastApproxQn"};
        const int n_draws = kind == kQn ? 2 * want : want;
        NL_RUN_HIP(hipMemsetAsync(d_state, 0, sizeof(CallState), stream));
        Launcher L(stream);
        draws(L, seed, true, 0, n_draws);
        const unsigned grid = (unsigned)((want + 255) / 256);
        if (kind == kMedian) L(locscale_gather_kernel<kMedian>, grid, 256, 0, data, pixels, d_raw, want, location, d_samples);
        else if (kind == kMad) L(locscale_gather_kernel<kMad>, grid, 256, 0, data, pixels, d_raw, want, location, d_samples);
        else L(locscale_gather_kernel<kQn>, grid, 256, 0, data, pixels, d_raw, want, location, d_samples);
        select(L, kind == kQn);
        NL_RUN_LAUNCHED(L);
        CallState s;
        if (const int rc = read_state(&s); rc != NL_OK) return rc;
        if (s.nan) return nan_error(names[kind], call, s.nan);
        *out = selected(s, kind == kQn);
        *consumed = (uint32_t)n_draws;
        return NL_OK;
    }

    // FastApproxBoundedMedian / FastApproxBoundedQn, in rounds of the stream up to the draw budget
    int bounded(bool qn, int call, uint32_t seed, float lo, float hi, float *out, uint32_t *consumed)
    {
        const char *fn = qn ? "FastApproxBoundedQn" : "FastApproxBoundedMedian";
        const int64_t budget = (int64_t)(qn ? 32 : 16) * want;
        const int round = qn ? round_qn : round_median;
        NL_RUN_HIP(hipMemsetAsync(d_state, 0, sizeof(CallState), stream));
        int64_t pos = 0;
        for (int r = 0; pos < budget; r++) {
            const int n = (int)std::min<int64_t>(round, budget - pos);
            const unsigned grid = (unsigned)((n + 255) / 256);
            Launcher L(stream);
            draws(L, seed, r == 0, r & 1, n);
            if (qn) {
                L(locscale_gather_bounded_kernel<true>, grid, 256, 0, data, pixels, d_raw, n, r == 0 ? 1 : 0, r & 1,
                  d_state, lo, hi, d_val, d_flags);
                L(locscale_compact_kernel<true>, 1, kCompactThreads, 0, d_val, d_flags, n, (uint32_t)pos,
                  (uint32_t)want, d_state, d_samples);
            } else {
                L(locscale_gather_bounded_kernel<false>, grid, 256, 0, data, pixels, d_raw, n, r == 0 ? 1 : 0, r & 1,
                  d_state, lo, hi, d_val, d_flags);
                L(locscale_compact_kernel<false>, 1, kCompactThreads, 0, d_val, d_flags, n, (uint32_t)pos,
                  (uint32_t)want, d_state, d_samples);
            }
            select(L, qn);             // (of use only once the samples are full: saves that round's second read-back)
            NL_RUN_LAUNCHED(L);
            CallState s;
            if (const int rc = read_state(&s); rc != NL_OK) return rc;
            pos += n;
            if (s.filled < (uint32_t)want) continue;
            if (s.nan) return nan_error(fn, call, s.nan);
            *out = selected(s, qn);
            *consumed = s.consumed;
            return NL_OK;
        }
        char bounds[96];
        snprintf(bounds, sizeof bounds, "[%g, %g]", (double)lo, (double)hi);
        return invalid(msg, std::string(fn) + " (sampling call " + std::to_string(call) + "): fewer than 1 in 16 draws within " +
                                bounds + ": " + std::to_string(budget) + " draws did not fill " + std::to_string(want) +
                                " samples (the reference would go on drawing)");
    }
};

// HistogramScaleLoc (:640-688) behind its bins, literally
void histogram_scale_loc(const std::vector<uint32_t> &bins, int64_t n, float mn, float value_to_bin, float *loc,
                         float *scale, nl_locscale_t *info)
{
    const uint32_t num_bins = kLocScaleBins;
    uint32_t peak_bin = 0, peak_count = 0;
    for (uint32_t bin = 1; bin < num_bins - 1; bin++)
        if (bins[bin] > peak_count) { peak_bin = bin; peak_count = bins[bin]; }
    *loc = mn + (float)peak_bin / value_to_bin;
    const uint32_t sigma_threshold = (uint32_t)((float)n * 0.6827f);
    uint32_t interval_limit = peak_bin;
    if (num_bins - 1 - peak_bin < interval_limit) interval_limit = num_bins - 1 - peak_bin;
    uint32_t cum = peak_count, reached = 0;
    float s = 0.5f * 1.0f / value_to_bin;
    if (cum < sigma_threshold) {
        for (uint32_t i = 1; i <= interval_limit; i++) {
            cum = cum + bins[peak_bin - i] + bins[peak_bin + i];
            s = 0.5f * (float)(2 * i + 1) / value_to_bin;
            reached = i;
            if (cum >= sigma_threshold) break;
        }
    }
    *scale = s;
    info->peak_bin = peak_bin;
    info->peak_count = peak_count;
    info->half_width = reached;
}

}  // namespace

int locscale_run(const float *d_data, int64_t npix, int estimator, int num_samples, const uint32_t *seeds, float mn,
                 float mx, LocScaleWork &w, hipStream_t stream, float *location, float *scale, nl_locscale_t *info,
                 std::string *msg)
{
    Sampler sm{d_data, (uint32_t)npix, estimator == NL_LSE_HISTOGRAM ? 4 : num_samples, stream, msg};
    NL_RUN_HIP(w.buf.reserve(sm.carve(nullptr), stream));
    sm.carve(w.buf.ptr);

    if (estimator == NL_LSE_HISTOGRAM) {
        if (mn == mx) {                                         // :642-644
            *location = mn;
            *scale = 0.0f;
            return NL_OK;
        }
        const float value_to_bin = (float)(kLocScaleBins - 1) / (mx - mn);
        NL_RUN_HIP(hipMemsetAsync(sm.d_bins, 0, sizeof(uint32_t) * (kLocScaleBins + 1), stream));
        Launcher L(stream);
        const int64_t quads = std::max<int64_t>(npix >> 2, 1);
        L(locscale_hist_kernel, (unsigned)std::min<int64_t>((quads + kHistThreads - 1) / kHistThreads, kHistBlocks),
          kHistThreads, 0, d_data, npix, mn, value_to_bin, sm.d_bins);
        NL_RUN_LAUNCHED(L);
        std::vector<uint32_t> bins(kLocScaleBins + 1);
        NL_RUN_HIP(hipMemcpyAsync(bins.data(), sm.d_bins, sizeof(uint32_t) * bins.size(), hipMemcpyDeviceToHost, stream));
        NL_RUN_HIP(hipStreamSynchronize(stream));
        if (bins[kLocScaleBins])
            return invalid(msg, "HistogramScaleLoc (stats.go:652-653): " + std::to_string(bins[kLocScaleBins]) +
                                    " pixels whose bin is outside [0, 4096) (a NaN pixel, or min / max that are not the frame's)");
        histogram_scale_loc(bins, npix, mn, value_to_bin, location, scale, info);
        return NL_OK;
    }

    int rc;
    if (estimator == NL_LSE_MEDIAN_MAD) {                       // :232-234
        float median, mad;
        if ((rc = sm.unbounded(kMedian, 0, seeds[0], 0.0f, &median, &info->draws[0])) != NL_OK) return rc;
        info->seeds_used = 1;
        if ((rc = sm.unbounded(kMad, 1, seeds[1], median, &mad, &info->draws[1])) != NL_OK) return rc;
        info->seeds_used = 2;
        *location = median;
        *scale = mad * 1.4826f;
        return NL_OK;
    }

    // FastApproxSigmaClippedMedianAndQn(data, 2, 2, epsilon, numSamples), :477-499
    const float sigma_low = 2.0f, epsilon = info->epsilon;
    float loc, sc, q;
    int call = 0;
    if ((rc = sm.unbounded(kMedian, call, seeds[call], 0.0f, &loc, &info->draws[call])) != NL_OK) return rc;
    info->seeds_used = ++call;
    if ((rc = sm.unbounded(kQn, call, seeds[call], 0.0f, &q, &info->draws[call])) != NL_OK) return rc;
    info->seeds_used = ++call;
    sc = q * 2.21914f;
    for (int i = 0;; i++) {
        const float low_bound = loc - sigma_low * sc, high_bound = loc + sigma_low * sc;
        float new_loc, new_scale;
        if ((rc = sm.bounded(false, call, seeds[call], low_bound, high_bound, &new_loc, &info->draws[call])) != NL_OK) return rc;
        info->seeds_used = ++call;
        if ((rc = sm.bounded(true, call, seeds[call], low_bound, high_bound, &q, &info->draws[call])) != NL_OK) return rc;
        info->seeds_used = ++call;
        new_scale = q * 2.21914f;
        new_scale = new_scale * 1.134f;
        info->iterations = i + 1;
        const bool converged = (float)(fabs((double)(new_loc - loc)) + fabs((double)(new_scale - sc))) <= epsilon;
        if (converged || i >= 10) {
            info->converged = converged ? 1 : 0;
            if ((rc = sm.unbounded(kQn, call, seeds[call], 0.0f, &q, &info->draws[call])) != NL_OK) return rc;
            info->seeds_used = ++call;
            *location = loc;
            *scale = q * 2.21914f;
            return NL_OK;
        }
        loc = new_loc;
        sc = new_scale;
    }
}

}  // namespace nl
