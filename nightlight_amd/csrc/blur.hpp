// blur.hpp -- OpGaussianBlur / OpUnsharpMask (internal/ops/stretch/stretch.go:339-424, internal/ops/stretch/usm.go) for
// the C ABI in nlstack_frame_stretch.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

// ApplyUnsharpMask's scalars (usm.go:134)
struct UsmParams {
    float gain, min, max, abs_threshold;
};

// per-handle device scratch, grown on demand
struct BlurWork {
    DevBuffer tmp;                   // the frame between the two passes (usm.go's tmp)
    DevBuffer taps;                  // the kernel, uploaded once per call
    size_t bytes() const { return tmp.bytes + taps.bytes; }
    void release() { tmp.release(); taps.release(); }
};

// A pass whose radius is at most this stages its source tile and the reflected halo in LDS; a larger one takes every
// tap from global memory.
constexpr int kBlurRowStagedRadius = 32;     // row pass: 16 rows x (256 + 2 * 32 + 4) floats = 20.25 KiB
constexpr int kBlurColStagedRadius = 24;     // column pass: 64 rows x 256 floats = 64 KiB, at least 16 output rows
constexpr int kBlurMaxRadius = 65536;        // GaussianKernel1D's radius search ends here (no frame of < 2^31 pixels holds more)

// GaussianKernel1D (usm.go:41-82) with the reference's fp32 / fp64 steps.  NL_ERR_INVALID_ARG with the site in *msg for
// a sigma the reference cannot handle: NaN, negative, zero, +Inf, one whose radius comes out -1 (make with a negative
// length) or beyond kBlurMaxRadius.
int gaussian_kernel_1d(float sigma, std::vector<float> &taps, std::string *msg);

// Convolve1DX then Convolve1DY (usm.go:85-114) with the n_taps taps at `taps` (host) on one whole width x height frame
// resident at d_data (width * height < 2^31), in place on `stream`; with usm, ApplyUnsharpMask (usm.go:134-149) of the
// frame and its blur instead.  n_taps is odd and positive.  A radius n_taps / 2 above width or height is
// NL_ERR_INVALID_ARG (one reflection leaves the range).  Returns NL_OK or an NL_ERR_* code with the message in *msg.
int blur_run(float *d_data, int width, int height, const float *taps, int n_taps, const UsmParams *usm, BlurWork &w,
             hipStream_t stream, std::string *msg);

}  // namespace nl
