// bayer.hpp -- launchers of bayer.hip (OpBadPixel's Bayer branch, OpDebayer) for the C ABI in nlstack_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nl {

enum BayerChannel { kBayerR = 0, kBayerG = 1, kBayerB = 2 };

// The pixels of one channel of a raw width x height mosaic, as CosmeticCorrectionBayer walks them
// (badpixels_bayer.go:64-351): R from (xo, yo), B from (xo+1, yo+1), both every other row and column; G in every row
// from yo, starting at xo+1, xo, xo+1, ... (colorOffsetX).  Channel row j, its k-th pixel: (row_x(j) + 2k, row_y(j)).
// The compact buffers of the correction hold channel row j at j * cstride.
struct BayerGeom {
    int width, height;     // the raw mosaic
    int green;             // 1 for G
    int x0, y0;            // pattern origin of the channel's walk
    int rows;              // channel rows
    int cols;              // pixels of the longest channel row
    int cstride;           // floats per compact row (cols rounded up to 64)
    int64_t count;         // channel pixels (the reference's deltaNum)
};

__host__ __device__ inline int bayer_row_y(const BayerGeom &g, int j) { return g.green ? g.y0 + j : g.y0 + 2 * j; }
__host__ __device__ inline int bayer_row_x(const BayerGeom &g, int j) { return g.green && !(j & 1) ? g.x0 + 1 : g.x0; }
__host__ __device__ inline int bayer_row_n(const BayerGeom &g, int j)
{
    const int x = bayer_row_x(g, j);
    return x < g.width ? (g.width - x + 1) >> 1 : 0;
}

// what the correction's launches hand each other on the device, and what the host reads back at the end
struct BayerParams {
    float mean, std;                 // of the channel's data - median (DeltaStatsBayer*)
    float lo, hi;                    // -sigma_low*std, sigma_high*std
    unsigned long long removed;      // numRemoved
};

struct BayerScratch {
    float *delta, *median;           // [rows * cstride] each, compact
    float *rowsum;                   // [rows]
    unsigned *removed;               // [bayer_replace_blocks(g)] replaced pixels per channel row
    BayerParams *params;
};

// channel xo / yo are the CFA offsets of getOffsets (debayer.go:26-37); width * height < 2^31
BayerGeom bayer_geom(int width, int height, int channel, int xo, int yo);
int64_t bayer_replace_blocks(const BayerGeom &g);

// CosmeticCorrectionBayer (badpixels_bayer.go:26-351) in place on one raw frame; any sigma (a negative one too)
hipError_t launch_bayer_correct(float *data, const BayerGeom &g, float sigma_low, float sigma_high,
                                const BayerScratch &s, hipStream_t stream);
// DebayerBilinear (debayer.go:41-263): out[row * out_stride + col] for the (width-xo)&~1 x (height-yo)&~1 plane
hipError_t launch_debayer(const float *data, int width, int height, int channel, int xo, int yo, float *out,
                          int64_t out_stride, hipStream_t stream);

}  // namespace nl
