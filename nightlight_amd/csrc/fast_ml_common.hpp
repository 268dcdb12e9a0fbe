// fast_ml_common.hpp -- building blocks of the multi-lane kernels (2 or 4 adjacent lanes
// share one pixel, 128 samples per lane): DPP quad permutes and reductions, the cross-lane
// bitonic merge, rank lookups, and the gather that ends with lane r holding the global sorted
// ranks [128r, 128r+128).  Used by stack_fast_ml.hip (sigma / winsor / median) and
// stack_linfit.hip (linear fit beyond 128 frames).  The median and MAD-sigma kernels of 513 ... 2048 frames
// (stack_fast_ml_deep.hip) run the same blocks on 8 or 16 lanes per pixel: half a DPP row or a whole one.
#pragma once
#include "fast_common.hpp"

namespace nl {

template <int CTRL>
__device__ __forceinline__ float dpp_f(float x)
{
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), CTRL, 0xF, 0xF, true));
}
template <int CTRL>
__device__ __forceinline__ int dpp_i(int x)
{
    return __builtin_amdgcn_mov_dpp(x, CTRL, 0xF, 0xF, true);
}
constexpr int kSwap1 = 0xB1;   // quad_perm [1,0,3,2]: partner = lane ^ 1
constexpr int kSwap2 = 0x4E;   // quad_perm [2,3,0,1]: partner = lane ^ 2
constexpr int kMirror = 0x1B;  // quad_perm [3,2,1,0]: partner = 3 - lane
// 8 and 16 lanes per pixel: partners within a row of 16 lanes
constexpr int kMirror8 = 0x141;   // row_half_mirror: partner = 7 - lane within 8
constexpr int kMirror16 = 0x140;  // row_mirror: partner = 15 - lane within 16
constexpr int kSwap8 = 0x128;     // row_ror:8: partner = lane ^ 8
// lane ^ 4 is no DPP control of this ISA: ds_swizzle_b32 in bit-mask mode, swizzle(SWAP,4) (and 0x1F, or 0, xor 4) --
// one instruction of the LDS crossbar (no LDS memory) where DPP would take two bank-masked row shifts
constexpr int kSwap4 = -4;
constexpr int kSwizzleSwap4 = 0x101F;

// the value of lane CTRL's partner: a DPP move, or the swizzle for kSwap4
template <int CTRL>
__device__ __forceinline__ float partner_f(float x)
{
    if constexpr (CTRL == kSwap4) return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(x), kSwizzleSwap4));
    else return dpp_f<CTRL>(x);
}

// 8 and 16 lanes per pixel: the lane's role computed anew from the lane's index in its wave (the lane counts divide 64 and
// the workgroup), three VALU operations where it is called.  The 128 samples and the networks' temporaries leave no
// register to spare between two uses of a role that lie a whole sort apart, and a value that cannot be kept is not spilled.
__device__ __forceinline__ int fresh_lane()
{
    int l;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
    return l;
}
template <int LPP>
__device__ __forceinline__ int fresh_role()
{
    static_assert(LPP == 8 || LPP == 16, "lanes per pixel");
    return fresh_lane() & (LPP - 1);
}

// sums / ors over the LPP lanes of a pixel; every lane gets the same bits
template <int LPP>
__device__ __forceinline__ float quad_sum(float x)
{
    static_assert(LPP == 2 || LPP == 4 || LPP == 8 || LPP == 16, "lanes per pixel");
    x = x + dpp_f<kSwap1>(x);
    if constexpr (LPP >= 4) x = x + dpp_f<kSwap2>(x);
    // (all four lanes of a quad hold the same bits now, so any lane of the other quad is a partner; likewise at 16)
    if constexpr (LPP >= 8) x = x + dpp_f<kMirror8>(x);
    if constexpr (LPP == 16) x = x + dpp_f<kMirror16>(x);
    return x;
}
template <int LPP>
__device__ __forceinline__ int quad_sum(int x)
{
    x = x + dpp_i<kSwap1>(x);
    if constexpr (LPP >= 4) x = x + dpp_i<kSwap2>(x);
    if constexpr (LPP >= 8) x = x + dpp_i<kMirror8>(x);
    if constexpr (LPP == 16) x = x + dpp_i<kMirror16>(x);
    return x;
}
template <int LPP>
__device__ __forceinline__ int quad_or(int x)
{
    x = x | dpp_i<kSwap1>(x);
    if constexpr (LPP >= 4) x = x | dpp_i<kSwap2>(x);
    if constexpr (LPP >= 8) x = x | dpp_i<kMirror8>(x);
    if constexpr (LPP == 16) x = x | dpp_i<kMirror16>(x);
    return x;
}

// the pixel's lane `R`, in every lane of the pixel
template <int LPP, int R>
__device__ __forceinline__ int quad_bcast(int x)
{
    if constexpr (LPP == 2) return dpp_i<R == 0 ? 0xA0 : 0xF5>(x);            // quad_perm [0,0,2,2] / [1,1,3,3]
    else return dpp_i<R == 0 ? 0x00 : (R == 1 ? 0x55 : (R == 2 ? 0xAA : 0xFF))>(x);
}

// in-lane half-cleaners of a bitonic merge: distances NS/2 ... 1, ascending
template <int NS, int D, int CH = 32>
__device__ __forceinline__ void half_clean(float (&v)[NS])
{
    if constexpr (D >= 1) {
        static_chunks<0, NS / 2, CH>([&](auto T) NL_INL {
            constexpr int t = decltype(T)::value;
            constexpr int i = ((t & ~(D - 1)) << 1) | (t & (D - 1));
            constexpr int l = i | D;
            const float lo = fminf(v[i], v[l]);
            const float hi = fmaxf(v[i], v[l]);
            v[i] = lo;
            v[l] = hi;
        });
        half_clean<NS, (D >> 1), CH>(v);
    }
}

// The last merge of the zonal kernels: only the KEEP lowest and KEEP highest
// positions of the lane must end up sorted (clip zones, median window); all
// other positions are only ever summed, so they merely have to hold the right
// SET.  A half-cleaner block that cannot reach either end is skipped:
// 224 instead of 448 compare-exchanges for NS = 128, KEEP = 16.
template <int NS, int D, int KEEP, int CH = 32>
__device__ __forceinline__ void half_clean_ends(float (&v)[NS])
{
    if constexpr (D >= 1) {
        static_chunks<0, NS / 2, CH>([&](auto T) NL_INL {
            constexpr int t = decltype(T)::value;
            constexpr int i = ((t & ~(D - 1)) << 1) | (t & (D - 1));
            constexpr int l = i | D;
            constexpr int blk = i & ~(2 * D - 1);                 // this comparator's block [blk, blk + 2D)
            if constexpr (blk < KEEP || blk + 2 * D > NS - KEEP) {
                const float lo = fminf(v[i], v[l]);
                const float hi = fmaxf(v[i], v[l]);
                v[i] = lo;
                v[l] = hi;
            }
        });
        half_clean_ends<NS, (D >> 1), KEEP, CH>(v);
    }
}

// cross-lane stage against the partner selected by CTRL; MIRROR: element i
// meets the partner's element NS-1-i (first stage of merging two ascending
// runs), else element i meets element i (half-cleaner at lane distance)
template <int NS, int CTRL, bool MIRROR>
__device__ __forceinline__ void cross_stage(float (&v)[NS], bool keep_min)
{
    // min(x, y) = med3(x, y, -Inf), max(x, y) = med3(x, y, +Inf): one VALU op per
    // element whichever side of the exchange the lane is on (no NaN can occur here)
    const float side = keep_min ? -__builtin_inff() : __builtin_inff();
    if constexpr (MIRROR) {
        static_chunks<0, NS / 2, 16>([&](auto I) NL_INL {
            constexpr int i = decltype(I)::value;
            constexpr int j = NS - 1 - i;
            const float pj = partner_f<CTRL>(v[j]);
            const float pi = partner_f<CTRL>(v[i]);
            v[i] = __builtin_amdgcn_fmed3f(v[i], pj, side);
            v[j] = __builtin_amdgcn_fmed3f(v[j], pi, side);
        });
    } else {
        static_chunks<0, NS, 32>([&](auto I) NL_INL {
            constexpr int i = decltype(I)::value;
            const float pv = partner_f<CTRL>(v[i]);
            v[i] = __builtin_amdgcn_fmed3f(v[i], pv, side);
        });
    }
}

// value at global sorted rank g (all lanes of the pixel receive it).  TOPW/BOTW
// restrict the lookup to the last TOPW registers of lane `lo_role` and the first
// BOTW registers of lane lo_role+1 (the only places g can be in the zonal
// passes); TOPW = BOTW = NS searches everything.
template <int LPP, int NS, int TOPW, int BOTW>
__device__ __forceinline__ float pick_rank(const float (&v)[NS], int g, int role, int lo_role)
{
    const int local = g - role * NS;
    float r = 0.0f;
    bool hit = false;
    if constexpr (TOPW >= NS) {
        hit = (unsigned)local < (unsigned)NS;
        r = pick<0, NS>(v, local);
    } else {
        const bool top = role == lo_role && local >= NS - TOPW && local < NS;
        const bool bot = role == lo_role + 1 && local >= 0 && local < BOTW;
        const float rt = pick<NS - TOPW, NS>(v, local);
        const float rb = pick<0, BOTW>(v, local);
        hit = top || bot;
        r = top ? rt : rb;
    }
    return __int_as_float(quad_or<LPP>(hit ? __float_as_int(r) : 0));
}

// ZONAL / generic exactly as in stack_fast.hip; LPP lanes per pixel.
// Sort every lane's column and merge the LPP runs of a pixel: afterwards lane r holds the global
// ranks [r*NS, r*NS+NS).  ENDS_ONLY: the last merge orders only the KEEP lowest / highest ranks
// of every lane (see half_clean_ends).
// NSL: positions [NSL, NS) of every lane are known to hold +Inf (frames the stack does not have: the caller's
// frame-count class), so the in-lane sort is the network of NSL positions -- 1 100 instead of 2 184 operations
// for a 300-frame stack on four lanes
template <int LPP, int NS, bool ENDS_ONLY, int KEEP = 16, int CH = 32, int NSL = NS>
__device__ __forceinline__ void ml_sort_merge(float (&v)[NS], int role)
{
    sort_network<NSL, true, NS>(v);
    if constexpr (LPP >= 8) role = fresh_role<LPP>();
    // ---- merge the LPP sorted runs: lane r ends up with ranks [r*NS, r*NS+NS) ----
    // (zonal: the final half-cleaners only order the ends of each lane, see half_clean_ends)
    static_assert(kZone + kPadMax <= KEEP, "zones must lie inside the sorted ends");
    cross_stage<NS, kSwap1, true>(v, (role & 1) == 0);
    // the in-lane half-cleaners run as 2-/3-input operations too (FusedBitonic, sort_tables.inc: the
    // 0-1 analysis over bitonic inputs fuses 30 % of the instructions away)
    static_assert(LPP <= 4 || (NS == 128 && !ENDS_ONLY), "8 and 16 lanes per pixel: full sort of 128 samples per lane");
    if constexpr (NS == 128 && (KEEP == 16 || KEEP == 32)) {
        if constexpr (ENDS_ONLY && LPP == 2) run_network<FusedBitonic<NS, KEEP>, NS>(v);
        else                             run_network<FusedBitonic<NS, 0>, NS>(v);
        if constexpr (LPP == 4) {
            cross_stage<NS, kMirror, true>(v, role < 2);
            cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
            if constexpr (ENDS_ONLY) run_network<FusedBitonic<NS, KEEP>, NS>(v);
            else                 run_network<FusedBitonic<NS, 0>, NS>(v);
        }
        if constexpr (LPP >= 8) {
            // two runs of 2 lanes -> one of 4, as above; then two of 4 -> one of 8: mirrored against lane 7 - r, half-cleaners
            // at lane distance 2 and 1, the in-lane network
            // (the role anew behind every in-lane network: fresh_role)
            role = fresh_role<LPP>();
            cross_stage<NS, kMirror, true>(v, (role & 2) == 0);
            cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
            run_network<FusedBitonic<NS, 0>, NS>(v);
            role = fresh_role<LPP>();
            cross_stage<NS, kMirror8, true>(v, (role & 4) == 0);
            cross_stage<NS, kSwap2, false>(v, (role & 2) == 0);
            cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
            run_network<FusedBitonic<NS, 0>, NS>(v);
        }
        if constexpr (LPP == 16) {
            // two runs of 8 lanes -> one of 16: mirrored against lane 15 - r, then distances 4, 2 and 1
            role = fresh_role<LPP>();
            cross_stage<NS, kMirror16, true>(v, (role & 8) == 0);
            cross_stage<NS, kSwap4, false>(v, (role & 4) == 0);
            cross_stage<NS, kSwap2, false>(v, (role & 2) == 0);
            cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
            run_network<FusedBitonic<NS, 0>, NS>(v);
        }
    } else {
        if constexpr (ENDS_ONLY && LPP == 2) half_clean_ends<NS, NS / 2, KEEP, CH>(v);
        else                             half_clean<NS, NS / 2, CH>(v);
        if constexpr (LPP == 4) {
            cross_stage<NS, kMirror, true>(v, role < 2);
            cross_stage<NS, kSwap1, false>(v, (role & 1) == 0);
            if constexpr (ENDS_ONLY) half_clean_ends<NS, NS / 2, KEEP, CH>(v);
            else                 half_clean<NS, NS / 2, CH>(v);
        }
    }
}

// Gather one pixel's frames into the LPP lanes that share it (128 per lane), sort every
// lane's column and merge the runs: afterwards lane r holds global ranks [r*NS, r*NS+NS)
// (+Inf for missing samples at the top).  Returns the number of valid samples of the pixel.
// ENDS_ONLY: the last merge orders only the KEEP lowest / highest ranks of every lane.
// The gather alone: the lane's samples as loaded, NaN and missing frames as +Inf; returns the number of valid
// samples of the PIXEL (all its lanes).
// KPAD0 / NLOAD (frame-count classes, stack_fast_mlz_impl.hpp): positions below KPAD0 always hold a frame, positions from
// NLOAD on never do -- they are +Inf without a load -- and only the few in between depend on the frame count: those become
// +Inf directly and stay out of the finiteness test, so that a wave without NaN samples skips the NaN count although its
// lanes are not full (with the defaults every lane of a stack that does not fill its lanes takes the 640-instruction
// count in every wave).
// NT: cache policy nt for the loads -- only where a wave reads WHOLE 128-byte lines of a frame and nobody reads them again:
// two lanes per pixel (32 pixels per wave).  Measured on the padded stride: median 256 frames
// 4.11 -> 3.84 ms, sigma 256 frames 4.62 -> 4.55; four lanes per pixel (64 bytes per frame and wave, the neighbouring wave
// takes the other half of the line through L1 / L2) LOSE 5 % with it, and so does the MAD kernel (+ 14 %: it reads the
// column a second time out of the MALL).
template <int LPP, int NS, int KPAD0 = NS / 2, int NLOAD = NS, bool NT = false>
__device__ __forceinline__ int ml_gather_raw(const float *frames, int64_t stride, int N, bool on, int64_t pix,
                                             int role, float (&v)[NS])
{
    static_assert(KPAD0 <= NLOAD && NLOAD <= NS, "positions");
    // (8 / 16 lanes per pixel serve 513 ... 1024 / 1025 ... 2048 frames: more than LPP * NS / 2, so the defaults' invariant
    // -- only positions k >= NS / 2 can lack a frame -- holds; LPP * frame_bytes < 2^31 is deep_ml_supported's bound)
    constexpr bool CLASS = !(KPAD0 == NS / 2 && NLOAD == NS);
    int nan_cnt = 0;
    int spad = NS - NLOAD;                                   // positions of this lane without a frame
    {
        // Frames are dealt round-robin: lane role r takes frames r, r+LPP, ...
        // (any split works, the column is sorted afterwards).  Buffer loads: one
        // scalar descriptor per register index k covering frames k*LPP .. k*LPP+LPP-1,
        // per-lane byte offset = pixel + role * frame.  The descriptor's size is
        // cut at the last existing frame, so a lane whose frame k*LPP+role does
        // not exist reads out of range -- the hardware returns 0 without touching
        // memory -- and the position is marked missing below.  No per-lane
        // addresses, no branches; descriptors are scalar work.
        int frame_bytes = (int)(stride * (int64_t)sizeof(float));           // LPP*frame_bytes < 2^31 (dispatch)
        // opaque per trip: otherwise the 128 descriptors are hoisted out of the
        // item loop as loop invariants and spilled
        asm volatile("" : "+s"(frame_bytes));
        const int voff = (int)((unsigned)(on ? pix : 0) * 4u) + role * frame_bytes;
        static_chunks<0, NLOAD, 4>([&](auto K) NL_INL {
            constexpr int k = decltype(K)::value;
            const int avail = min(max(N - k * LPP, 0), LPP);                // frames this descriptor covers
            const char *gb = reinterpret_cast<const char *>(frames) + (int64_t)(k * LPP) * frame_bytes;
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(gb), 0, avail * frame_bytes, 0x00020000);
            v[k] = __int_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, 0, NT ? 2 : 0));
        });
        static_range<NLOAD, NS>([&](auto K) NL_INL { v[decltype(K)::value] = __builtin_inff(); });
        int lastp = opaque(N - 1) - role;
        float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f;
        if constexpr (CLASS) {
            // frame k*LPP+role >= N: no frame -> +Inf, counted, kept out of the sum below
            float tp = 0.0f;
            static_range<KPAD0, NLOAD>([&](auto K) NL_INL {
                constexpr int k = decltype(K)::value;
                const int pad = (lastp - k * LPP) >> 31;                       // all ones: no frame
                tp += __int_as_float(__float_as_int(v[k]) & ~pad);
                v[k] = __int_as_float((__float_as_int(v[k]) & ~pad) | (0x7f800000 & pad));
                spad -= pad;
            });
            static_chunks<0, KPAD0 / 4, 8>([&](auto K) NL_INL {
                constexpr int k = 4 * decltype(K)::value;
                t0 += v[k]; t1 += v[k + 1]; t2 += v[k + 2]; t3 += v[k + 3];
            });
            static_range<KPAD0 / 4 * 4, KPAD0>([&](auto K) NL_INL { t0 += v[decltype(K)::value]; });
            t0 += tp;
        } else {
            // frame k*LPP+role >= N: missing (NaN).  Only k >= KPAD0 can be affected:
            // this kernel is used for N > NT/2.
            static_chunks<KPAD0, NS, 8>([&](auto K) NL_INL {
                constexpr int k = decltype(K)::value;
                if constexpr ((k & 7) == 0) lastp = opaque(lastp);
                const int pad = (lastp - k * LPP) >> 31;                           // all ones -> NaN
                v[k] = __int_as_float(__float_as_int(v[k]) | pad);
            });
            // clean waves skip the NaN count (see gather_sorted in fast_common.hpp)
            static_chunks<0, NS / 4, 8>([&](auto K) NL_INL {
                constexpr int k = 4 * decltype(K)::value;
                t0 += v[k]; t1 += v[k + 1]; t2 += v[k + 2]; t3 += v[k + 3];
            });
        }
        const float total = (t0 + t1) + (t2 + t3);
        if (__any(!(__builtin_fabsf(total) < __builtin_inff()))) {
            static_chunks<0, NLOAD, 8>([&](auto K) NL_INL {
                constexpr int k = decltype(K)::value;
                nan_cnt = opaque(nan_cnt - ((0x7f800000 - (__float_as_int(v[k]) & 0x7fffffff)) >> 31));
                asm volatile("v_min_f32 %0, %0, %1" : "+v"(v[k]) : "v"(__builtin_inff()));   // NaN -> +Inf in place
            });
        }
    }
    return quad_sum<LPP>(NS - nan_cnt - spad);
}

template <int LPP, int NS, bool ENDS_ONLY, int KEEP = 16, int CH = 32, int NSL = NS, int KPAD0 = NS / 2, int NLOAD = NS, bool NT = false>
__device__ __forceinline__ int ml_gather_sorted(const float *frames, int64_t stride, int N, bool on, int64_t pix,
                                                int role, float (&v)[NS])
{
    const int n = ml_gather_raw<LPP, NS, KPAD0, NLOAD, NT>(frames, stride, N, on, pix, role, v);
    ml_sort_merge<LPP, NS, ENDS_ONLY, KEEP, CH, NSL>(v, role);
    return n;
}

}  // namespace nl
