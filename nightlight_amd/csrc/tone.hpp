// tone.hpp -- the per-pixel curves of the stretch command (OpNormalizeRange, OpStretchIterative's two pixel passes,
// OpMidtones, OpGamma, OpGammaPP, OpScaleBlack: internal/ops/stretch/stretch.go:40-335 over internal/fits/pixelops.go)
// and OpSave's quantisation to 16- or 8-bit gray (internal/fits/tiff16.go:108-135, writejpg.go:106-131) for the C ABI in
// nlstack_frame_stretch.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "../../include/nlstack.h"

namespace nl {

// what the kernels take: the loop constants the reference derives in front of its pixel loop, from its own arguments
// and in its own fp32 / fp64 steps (tone_args)
enum ToneOp { kToneAffine, kToneGamma, kTonePartialGamma, kToneMidtones, kToneShiftBlack };
struct ToneArgs {
    int op;                // ToneOp
    float a, b, c, d, e;   // affine: scale, offset; partial gamma: from, to, rescale1, rescale2; midtones: mid - 1,
                           // 2 mid - 1, mid, clipLow, scaler; shift black: black, scale
    double gg;             // gamma, partial gamma: float64(1.0f / g)
};

// The constants of curve t.  *noop: the operator's own guard holds (g == 1 of NL_TONE_GAMMA, stretch.go:240), nothing
// is to be computed.  An unknown kind is NL_ERR_INVALID_ARG with the message in *msg.
int tone_args(const nl_tone_t &t, ToneArgs *args, bool *noop, std::string *msg);

// The curve over the n floats at d_data, in place on `stream`: 16-byte loads and stores where d_data is 16-byte
// aligned, the same quads element by element where it is not (slot i of a dense handle whose pixel count is no multiple
// of 4).  With partial: the variant that also reduces the transformed values exactly as launch_min_sum_max would
// on them afterwards -- `blocks` workgroups, the same partition, {min, sum, max} per workgroup into partial[3 * blocks]
// -- seeded from the transformed element 0, which a one-lane launch puts into *seed first (the kernel itself
// overwrites data[0]).  Without: the plain variant, seed and blocks unused.
hipError_t launch_tone(float *d_data, int64_t n, const ToneArgs &args, float *seed, double *partial, int blocks,
                       hipStream_t stream);

// OpSave's pixel loop: gray = (d - min) * scale; NaN or < 0 -> 0; > 1 -> 1; with use_gamma float32(pow(float64(gray),
// gamma_inv)); then gray * 65535 (bits 16, two bytes per pixel, high byte first: image.Gray16.Pix) or gray * 255
// (bits 8: image.Gray.Pix) truncated.  n floats at d_data (16-byte loads where it is 16-byte aligned, else element by element)
// into n * bits / 8 bytes at d_out (8-byte aligned).
hipError_t launch_export_gray(const float *d_data, int64_t n, float min, float scale, bool use_gamma, double gamma_inv,
                              int bits, void *d_out, hipStream_t stream);

}  // namespace nl
