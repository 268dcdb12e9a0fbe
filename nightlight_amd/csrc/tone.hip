// tone.hip -- the per-pixel curves of the reference's stretch command and OpSave's quantisation for gfx950.
//   tone_kernel          internal/fits/pixelops.go:123-128  pfScaleOffset (ApplyScaleOffset, Normalize :143-147)
//                                                  :151-157  pfGamma
//                                                  :179-191  pfPartialGamma
//                                                  :214-229  pfMidtones
//                                                  :649-660  ShiftBlackToMove
//   export_gray_kernel   internal/fits/tiff16.go:108-135     WriteMonoTIFF16
//                        internal/fits/writejpg.go:106-131   WriteMonoJPG
// Every curve is the reference's expression, operation for operation, in fp32 without FMA and with IEEE division; the
// powers are the device's fp64 pow on the widened pixel, narrowed once.  The loop constants come from tone_args below,
// host code compiled without contraction like the kernels.  One HBM stream each, 256 lanes; 16-byte loads and stores
// where the pointer allows (VEC), the same quads element by element (4-byte alignment) where it does not: slot i of a handle whose pixel count
// is no multiple of 4 starts off a 16-byte boundary.
// The variant with statistics walks the frame in min_sum_max_kernel's partition and reduces what it writes, so the
// operator that follows needs no second pass for Stats.Min() / Mean() / Max().
#include "frame_common.hpp"
#include "launch_common.hpp"
#include "quad_common.hpp"
#include "tone.hpp"

namespace nl {

namespace {

template <int OP>
__device__ __forceinline__ float tone_pixel(float d, const ToneArgs &p)
{
    if constexpr (OP == kToneAffine) {
        return d * p.a + p.b;                                            // pixelops.go:126
    } else if constexpr (OP == kToneGamma) {
        return pow_f32(d, p.gg);                                         // :155
    } else if constexpr (OP == kTonePartialGamma) {
        if (d > p.a && d < p.b) {                                        // :185 (a NaN keeps its bits)
            const float dd = (d - p.a) * p.c;
            const float gamma_dd = pow_f32(dd, p.gg);
            return p.a + gamma_dd * p.d;
        }
        return d;
    } else if constexpr (OP == kToneMidtones) {
        float value = d * p.a / (p.b * d - p.c);                         // :220
        if (value < p.d) value = 0.0f;                                   // (a NaN falls through both tests)
        else if (value > 1.0f) value = 1.0f;
        return (value - p.d) * p.e;
    } else {
        // float32(math.Max(0, float64(x))), :657: NaN for a NaN, +0 for -0 and for every negative x
        const float x = (d - p.a) * p.b;
        if (x != x) return x;
        return x > 0.0f ? x : 0.0f;
    }
}

// f(data[0]) for the reduction's seed: tone_kernel<OP, true> overwrites data[0] while other lanes still start
template <int OP>
__global__ void tone_seed_kernel(const float *data, ToneArgs p, float *seed)
{
    *seed = tone_pixel<OP>(data[0], p);
}

// In place; STATS: the variant that reduces what it writes (quad_transform, quad_common.hpp)
template <int OP, bool STATS, bool VEC>
__global__ __launch_bounds__(256) void tone_kernel(float *data, int64_t n, ToneArgs p, const float *seed, double *partial)
{
    quad_transform<STATS, VEC>(data, n, [p](float d) { return tone_pixel<OP>(d, p); }, seed, partial);
}

// four pixels per lane into one 8-byte (16 bits, high byte first) or 4-byte store; the tail byte by byte
template <int BITS, bool GAMMA, bool VEC>
__global__ __launch_bounds__(256) void export_gray_kernel(const float *data, int64_t n, float min, float scale,
                                                          double gamma_inv, unsigned char *out)
{
    const int64_t quads = n >> 2;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (int64_t)gridDim.x * blockDim.x) {
        const float4 v = load_quad<VEC>(data, q);
        const unsigned c0 = gray_count<BITS, GAMMA>(v.x, min, scale, gamma_inv);
        const unsigned c1 = gray_count<BITS, GAMMA>(v.y, min, scale, gamma_inv);
        const unsigned c2 = gray_count<BITS, GAMMA>(v.z, min, scale, gamma_inv);
        const unsigned c3 = gray_count<BITS, GAMMA>(v.w, min, scale, gamma_inv);
        if constexpr (BITS == 16) {
            // bytes hi0 lo0 hi1 lo1 | hi2 lo2 hi3 lo3 as two little-endian words
            const unsigned w0 = (c0 >> 8) | ((c0 & 255u) << 8) | ((c1 >> 8) << 16) | ((c1 & 255u) << 24);
            const unsigned w1 = (c2 >> 8) | ((c2 & 255u) << 8) | ((c3 >> 8) << 16) | ((c3 & 255u) << 24);
            reinterpret_cast<uint2 *>(out)[q] = make_uint2(w0, w1);
        } else {
            reinterpret_cast<unsigned *>(out)[q] = c0 | (c1 << 8) | (c2 << 16) | (c3 << 24);
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (quads << 2) + threadIdx.x;
        const unsigned c = gray_count<BITS, GAMMA>(data[i], min, scale, gamma_inv);
        if constexpr (BITS == 16) {
            out[2 * i] = (unsigned char)(c >> 8);
            out[2 * i + 1] = (unsigned char)(c & 255u);
        } else {
            out[i] = (unsigned char)c;
        }
    }
}

// f(std::integral_constant<int, OP>) for the ToneOp op; false for any other value
template <class F>
bool with_tone_op(int op, F &&f)
{
    switch (op) {
    case kToneAffine:       f(std::integral_constant<int, kToneAffine>{}); return true;
    case kToneGamma:        f(std::integral_constant<int, kToneGamma>{}); return true;
    case kTonePartialGamma: f(std::integral_constant<int, kTonePartialGamma>{}); return true;
    case kToneMidtones:     f(std::integral_constant<int, kToneMidtones>{}); return true;
    case kToneShiftBlack:   f(std::integral_constant<int, kToneShiftBlack>{}); return true;
    default:                return false;
    }
}

}  // namespace

int tone_args(const nl_tone_t &t, ToneArgs *args, bool *noop, std::string *msg)
{
    ToneArgs a{};
    *noop = false;
    const float p0 = t.p[0], p1 = t.p[1], p2 = t.p[2];
    switch (t.kind) {
    case NL_TONE_SCALE_OFFSET:
        a.op = kToneAffine;
        a.a = p0;
        a.b = p1;
        break;
    case NL_TONE_NORMALIZE: {                      // pixelops.go:144-145, p = {min, max}
        a.op = kToneAffine;
        a.a = 1.0f / (p1 - p0);
        a.b = -p0 * a.a;
        break;
    }
    case NL_TONE_GAMMA:                            // :153, p = {g}
        a.op = kToneGamma;
        a.gg = (double)(1.0f / p0);
        *noop = p0 == 1.0f;                        // OpGamma.Apply, stretch.go:240
        break;
    case NL_TONE_PARTIAL_GAMMA:                    // :181-183, p = {from, to, g}
        a.op = kTonePartialGamma;
        a.a = p0;
        a.b = p1;
        a.gg = (double)(1.0f / p2);
        a.d = p1 - p0;
        a.c = 1.0f / a.d;
        break;
    case NL_TONE_MIDTONES: {                       // :216-218, p = {mid, black}
        a.op = kToneMidtones;
        a.a = p0 - 1.0f;
        a.b = 2.0f * p0 - 1.0f;
        a.c = p0;
        const float den = a.b * p1 - p0;
        a.d = p1 * a.a / den;                      // clipLow
        a.e = 1.0f / (1.0f - a.d);                 // scaler, clipHigh = 1
        break;
    }
    case NL_TONE_SHIFT_BLACK:                      // :653-654, p = {before, after}
        a.op = kToneShiftBlack;
        a.a = (p1 - p0) / (p1 - 1.0f);             // black
        a.b = 1.0f / (1.0f - a.a);                 // scale
        break;
    default:
        *msg = "unknown kind " + std::to_string(t.kind) + " (NL_TONE_SCALE_OFFSET ... NL_TONE_SHIFT_BLACK)";
        return NL_ERR_INVALID_ARG;
    }
    *args = a;
    return NL_OK;
}

hipError_t launch_tone(float *d_data, int64_t n, const ToneArgs &args, float *seed, double *partial, int blocks,
                       hipStream_t stream)
{
    if (n < 1 || !d_data || (partial && (!seed || blocks < 1))) return hipErrorInvalidValue;
    Launcher L(stream);
    const bool known = with_tone_op(args.op, [&](auto OP) {
        constexpr int op = decltype(OP)::value;
        with_bool(aligned16(d_data), [&](auto V) {
            constexpr bool vec = decltype(V)::value;
            if (partial) {
                L(tone_seed_kernel<op>, 1, 1, 0, d_data, args, seed);
                L(tone_kernel<op, true, vec>, blocks, 256, 0, d_data, n, args, seed, partial);
            } else {
                L(tone_kernel<op, false, vec>, quad_blocks(n), 256, 0, d_data, n, args, nullptr, nullptr);
            }
        });
    });
    return known ? L.err : hipErrorInvalidValue;
}

hipError_t launch_export_gray(const float *d_data, int64_t n, float min, float scale, bool use_gamma, double gamma_inv,
                              int bits, void *d_out, hipStream_t stream)
{
    if (n < 1 || !d_data || (reinterpret_cast<uintptr_t>(d_out) & 7) != 0 || (bits != 8 && bits != 16))
        return hipErrorInvalidValue;
    Launcher L(stream);
    with_bool(bits == 16, [&](auto WIDE) {
        with_bool(use_gamma, [&](auto G) {
            with_bool(aligned16(d_data), [&](auto V) {
                L(export_gray_kernel<decltype(WIDE)::value ? 16 : 8, decltype(G)::value, decltype(V)::value>,
                  quad_blocks(n), 256, 0, d_data, n, min, scale, gamma_inv, static_cast<unsigned char *>(d_out));
            });
        });
    });
    return L.err;
}

}  // namespace nl
