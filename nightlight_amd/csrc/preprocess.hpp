// preprocess.hpp -- launchers of preprocess.hip (OpCalibrate, OpBadPixel) for the C ABI in nlstack_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nl {

// pixels per workgroup of the bad-pixel classification (and the length of its list segment)
constexpr int kBpChunk = 1024;

// what the bad-pixel launches hand each other on the device, and what the host reads back at the end
struct BpParams {
    float mean, std;                 // Image.MedianDiffStats: mean and StdDev of the local-median differences
    float lo, hi;                    // thresholds -std*sigma_low, std*sigma_high
    unsigned long long removed;      // bad pixels
    unsigned chained;                // ... of them replaced by the ordered walk (bp_walk)
    unsigned pad;
};

struct BpScratch {
    float *diff;                     // [n]
    unsigned *seg;                   // [bp_blocks(n) * kBpChunk] per-workgroup lists of chained pixels
    unsigned *list;                  // [n] the chained pixels in index order
    unsigned *count, *offset;        // [bp_blocks(n)] each: list lengths, their exclusive prefix sums
    unsigned *removed;               // [bp_blocks(n)] bad pixels per workgroup
    BpParams *params;
    double *partial;                 // [stat_blocks]
    int stat_blocks;
};

int bp_blocks(int64_t n);

// out = Divide(Subtract(in, dark), flat, flat_max) elementwise (dark / flat may be NULL; out may equal in)
hipError_t launch_calibrate(const float *in, float *out, int64_t n, const float *dark, const float *flat,
                            float flat_max, hipStream_t stream);
// OpBadPixel (mono) in place on one whole width x height frame (width * height < 2^31); sigmas >= 0
hipError_t launch_badpixel(float *data, int width, int height, float sigma_low, float sigma_high, const BpScratch &s,
                           hipStream_t stream);

}  // namespace nl
