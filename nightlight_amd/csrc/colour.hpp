// colour.hpp -- the steps of the reference's rgb / lrgb command whose arithmetic is written out in its own source, on
// three planes resident in a handle, for the C ABI in nlstack_frame_rgb.hip:
//   internal/fits/rgb.go:43-78        NewRGBFromChannels, getCommonNormalizationFactors
//                       :94-149       SetBlackWhitePoints, setBlackWhitePoints
//                       :153-219      findDarkestBlock
//                       :223-281      meanStarIntensity
//   internal/fits/pixelops.go:441-550 pf3ChanChroma, pf3ChanNeutralizeBackground, pf3ChanChromaForHues, pf3ChanRotateColors
//                            :679-692 ScaleOffsetClampRGB
//   internal/fits/tiff16.go:45-91     WriteTIFF16
//   internal/fits/writejpg.go:43-89   WriteJPG
// The planes are three slots of one handle: three pointers, since slots are not contiguous (padded stride).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/nlstack.h"
#include "dev_memory.hpp"

namespace nl {

struct Planes { float *p[3]; };

// getCommonNormalizationFactors (rgb.go:65-78): strict compares from channel 0 on, mult = 1 / (max - min) in fp32
void rgb_normalization(const float mins[3], const float maxs[3], float *min, float *mult);
// setBlackWhitePoints' scalar part (rgb.go:125-145) in fp32, operation for operation
void rgb_balance_coeffs(nl_rgb_t cur_shadows, nl_rgb_t cur_highlights, nl_rgb_t target_shadows,
                        nl_rgb_t target_highlights, float alpha[3], float beta[3]);

// dst[j] = (src[j] - min) * mult over n floats (rgb.go:58); dst may be src
hipError_t launch_combine(float *d_dst, const float *d_src, int64_t n, float min, float mult, hipStream_t stream);

// ScaleOffsetClampRGB over the three planes of n floats in one launch, in place.  With partial: the variant that also
// reduces what it writes as launch_tone does, plane c into partial[3 * blocks * c ...] seeded from seed[c], which a
// three-lane launch fills first.
hipError_t launch_rgb_clamp(Planes planes, int64_t n, const float alpha[3], const float beta[3], float *seed,
                            double *partial, int blocks, hipStream_t stream);

// findDarkestBlock's geometry (rgb.go:158-163) in the reference's int32 / float32 arithmetic
struct BlockGrid {
    int32_t x_first, x_last, y_first, y_last;   // xBlockFirst ... yBlockLast
    int32_t nbx, nby;                           // blocks the loops visit (0: none)
    float inv_block_pixels;
};
BlockGrid darkest_block_grid(int width, int height, int block, float border);
// the block means {r, g, b} of every block the loops visit, row-major, into d_means[3 * nbx * nby]; direct: no strip
// is staged in LDS (a developer switch: the results are the same)
hipError_t launch_block_means(Planes planes, int width, const BlockGrid &g, int block, bool direct, float *d_means,
                              hipStream_t stream);
// the scan l = (r + g + b) / 3, l < lMin in row-major block order (rgb.go:211-214)
nl_rgb_t darkest_block_scan(const float *means, int64_t n_blocks);

// one star's sums over its disc (rgb.go:238-269)
struct StarSum { float r, g, b; int32_t pixels; };
// one lane per star of d_stars[n]: the disc loop of meanStarIntensity in its own order
hipError_t launch_star_sums(Planes planes, int width, int height, const nl_star_t *d_stars, int n, nl_rgb_t clip,
                            StarSum *d_sums, hipStream_t stream);
// sStart / sEnd (rgb.go:226-227; Go's int is 64 bits)
void star_range(int n_stars, float skip_bright, float skip_dim, int64_t *s_start, int64_t *s_end);
// hfrR of one star (rgb.go:239-240)
int32_t star_hfr_radius(float hfr);
// the fold in star order and the normalisation (rgb.go:272-280)
nl_rgb_t star_mean(const StarSum *sums, int n);

// the four steps of pixelops.go:441-550 on planes {h, c, l}; false for an unknown kind
hipError_t launch_chroma(Planes planes, int64_t n, const nl_chroma_t &op, hipStream_t stream);
bool chroma_kind_known(int kind);

// WriteTIFF16 / WriteJPG's pixel loop: n pixels of three planes into n * (bits == 16 ? 8 : 4) bytes at d_out (16-byte
// aligned): R G B A, big-endian uint16 with A = 0xFFFF, or bytes with A = 255
hipError_t launch_export_rgb(Planes planes, int64_t n, float min, float scale, bool use_gamma, double gamma_inv, int bits,
                             void *d_out, hipStream_t stream);

// device scratch of the colour steps: statistics partials and seeds of three planes, block means, stars and star sums
struct ColourWork {
    DevBuffer stats, means, stars;
    size_t bytes() const { return stats.bytes + means.bytes + stars.bytes; }
    void release() { stats.release(); means.release(); stars.release(); }
};

}  // namespace nl
