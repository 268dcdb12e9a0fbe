// deband.hpp -- OpDebandHoriz / OpDebandVert (internal/ops/pre/banding.go:61-270) and OpBin's NewImageBinNxN
// (internal/fits/fits.go:163-195) for the C ABI in nlstack_frame_pre.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

struct DebandParams {
    float percentile;                // in (0, 100): the operators' own guards are the caller's no-ops
    int window;                      // horiz: > 0 (guarded); vert: <= 0 is the reference's panic
    float threshold;                 // MaxFloat32 when sigma == 0, else location + sigma * scale
};

// per-handle device scratch, grown on demand
struct DebandWork {
    DevBuffer buf;                   // percentile and count of every row / column, the factors
    DevBuffer transposed;            // vert: the frame transposed, a bit copy
    DevBuffer stage;                 // rows of more than kDebandLdsSamples samples: their keys, re-read by every pass
    size_t bytes() const { return buf.bytes + transposed.bytes + stage.bytes; }
    void release() { buf.release(); transposed.release(); stage.release(); }
};

constexpr int kDebandLdsSamples = 16384;     // a row of up to this many samples is selected in LDS (64 KiB of keys)

// Apply of OpDebandHoriz (cols == false) or OpDebandVert (cols == true) after its guard, on one whole width x height
// frame resident at d_data (width * height < 2^31), in place on `stream`.  *lowest / *highest: the factors' range as
// the reference logs it.  Returns NL_OK or an NL_ERR_* code with the message in *msg.
int deband_run(float *d_data, int width, int height, bool cols, const DebandParams &p, DebandWork &w,
               hipStream_t stream, float *lowest, float *highest, std::string *msg);

// NewImageBinNxN: d_out[(height / n) x (width / n)] from d_in[height x width], n >= 2, both shapes non-empty
hipError_t launch_bin(const float *d_in, int width, int height, int n, float *d_out, hipStream_t stream);

}  // namespace nl
