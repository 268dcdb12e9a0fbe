// wclip_common.hpp -- the accumulation of the weighted clip pass whose weights follow their frames
// (include/nlstack_wclip.h, an extension): ONE function, called sample by sample in ascending frame index by both
// engines -- the streaming kernel of stack_clip_weighted.hip under the recorded thresholds, and the column kernel's
// <follow> instantiations (stack_exact.hip) under the closed interval of their survivors -- so that the two give the
// same bits by construction.
#pragma once
#include "stack_kernels.h"

namespace nl {

// what one pixel accumulates
struct WclipAcc {
    float num = 0.0f, den = 0.0f;     // sum of v_k * w_k and of w_k over the survivors, in frame order
    int lo = 0, hi = 0;               // samples out on the low / on the high side
    int last = 0;                     // ... of them in the last round on record
    int kept = 0;                     // survivors
};

// A round that rejects nothing: what stands in for the rounds a pixel does not have
__device__ __forceinline__ float2 wclip_no_round() { return make_float2(-__builtin_inff(), __builtin_inff()); }

// One sample of frame k.  The sample walks the rounds front[0 .. R-1] and then `last` in order: v < lo_r counts low and
// the sample is out, else v > hi_r counts high and the sample is out, otherwise it goes to the next round; a sample that
// passes every round is in: num += v * w; den += w (fp32, never fused: StackMeanWeighted's arithmetic, stack.go:343-364).
// NaN is no sample (stack.go:380-387); a NaN threshold rejects nothing, as in the reference.  `last` is the round behind
// which the record ends: acc.last counts what IT removes.  R: front rounds in registers (compile-time indices only;
// wclip_no_round() where a pixel has fewer); R = 0: front is not read.
// (The flags are integers, not bools: 32 samples' worth of wave masks would not fit the scalar registers.)
template <int R>
__device__ __forceinline__ void wclip_take(float v, float w, const float2 *front, float2 last, WclipAcc &acc)
{
    int in = (v == v) ? 1 : 0;                    // still in: a sample, and out in no round so far
    auto round = [&](float2 b, int &lo_out, int &hi_out) {
        lo_out = (v < b.x) ? in : 0;
        hi_out = (v > b.y) ? in - lo_out : 0;     // else if
        in -= lo_out + hi_out;
        acc.lo += lo_out;
        acc.hi += hi_out;
    };
    int l, h;
#pragma unroll
    for (int r = 0; r < R; r++) round(front[r], l, h);
    round(last, l, h);
    acc.last += l + h;
    acc.kept += in;
    const float num = __fadd_rn(acc.num, __fmul_rn(v, w)), den = __fadd_rn(acc.den, w);
    acc.num = in ? num : acc.num;
    acc.den = in ? den : acc.den;
}

}  // namespace nl
