// background.hpp -- background extraction (OpBackExtract: pre.NewBackground + Background.Subtract / Render,
// internal/ops/pre/background.go:68-462) for the C ABI in nlstack_frame_pre.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

struct BackParams {
    int grid;                        // GridSize > 0 (GridSize <= 0 is the caller's no-op)
    float hfr_factor, sigma;
    int clip;                        // Clip; <= 0: no clipping
};

// per-handle device scratch, grown on demand
struct BackWork {
    DevBuffer buf;                   // cell rectangles, star lists, cell results, grid, Subtract tables
    DevBuffer stage;                 // the large-cell path's star-masked samples (one float per pixel at most)
    DevBuffer render;                // the rendered background of background_host
    size_t bytes() const { return buf.bytes + stage.bytes + render.bytes; }
    void release() { buf.release(); stage.release(); render.release(); }
};

// NewBackground + Subtract on one whole width x height frame resident at d_data (width * height < 2^31), in place on
// `stream`.  background_host (NULL or width * height floats): the Render() image; cells_out: the first
// min(cells, cells_capacity) smoothed cell values.  Returns NL_OK or an NL_ERR_* code with the message in *msg.
int back_extract_run(float *d_data, int width, int height, const BackParams &p, const nl_star_t *stars, int n_stars,
                     BackWork &w, hipStream_t stream, float *background_host, float *cells_out, int cells_capacity,
                     nl_background_t *info, std::string *msg);

}  // namespace nl
