// stars.hpp -- star detection (star.FindStars, internal/star/findstars.go:59-103) for the C ABI in nlstack_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

struct StarParams {
    float location, scale;           // f.Stats.Location() / Scale(), as OpStarDetect.Apply passes them
    float star_sig, bp_sigma, star_in_out;
    int radius;                      // >= 0
    float diff_std;                  // f.MedianDiffStats.StdDev(); NaN: MedianDiffStats == nil
};

// per-handle device scratch, grown on demand
struct StarWork {
    DevBuffer buf;                   // candidate segments, list, flags, thresholds
    DevBuffer stars;                 // star lists of the centroid and HFR stages
    size_t bytes() const { return buf.bytes + stars.bytes; }
    void release() { buf.release(); stars.release(); }
};

// FindStars on one whole width x height frame resident at d_data (width * height < 2^31), on `stream`.  d_partial:
// stat_blocks doubles of scratch.  Returns NL_OK or an NL_ERR_* code with the message in *msg.
int find_stars_run(const float *d_data, int width, int height, const StarParams &p, StarWork &w, double *d_partial,
                   int stat_blocks, hipStream_t stream, std::vector<nl_star_t> &stars, float *sum_of_shifts,
                   float *avg_hfr, std::string *msg);

}  // namespace nl
