// locscale.hpp -- Stats.Location() / Scale() (internal/stats/stats.go:225-244): the sampling estimators LSEMedianMAD
// and LSESCMedianQn (:336-364, :401-410, :436-499), bit-exact given the seeds, and LSEHistogram (:640-688), for the C
// ABI in nlstack_frame.hip.  (LSEMeanStdDev comes from the reductions of frame_stats.hip.)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

constexpr int kLocScaleBins = 4096;              // stats.go:241
constexpr int kLocScaleMaxSamples = 1 << 20;     // the jump table of the draw stream covers a round of 2.5 x this many draws

// per-handle device scratch, grown on demand
struct LocScaleWork {
    DevBuffer buf;                   // call state, the round's raw draws, values and flags, the samples, the bins
    size_t bytes() const { return buf.bytes; }
    void release() { buf.release(); }
};

// Estimator NL_LSE_MEDIAN_MAD, NL_LSE_SC_MEDIAN_QN or NL_LSE_HISTOGRAM on the npix (2 <= npix < 2^31) floats resident
// at d_data, on `stream`; mn / mx: Stats.Min() / Max().  seeds: 2 / 25 / none, all nonzero.  info is filled (never
// null here).  Returns NL_OK or an NL_ERR_* code with the message in *msg; the stream is idle either way.
int locscale_run(const float *d_data, int64_t npix, int estimator, int num_samples, const uint32_t *seeds, float mn,
                 float mx, LocScaleWork &w, hipStream_t stream, float *location, float *scale, nl_locscale_t *info,
                 std::string *msg);

}  // namespace nl
