// wave_lists.hpp -- the steps with which every stack kernel ends a pixel or a pass: the wave's
// sum, the append of the lanes that cannot finish a pixel to a hand-over list, and where and how clip totals are added.
// No state of its own; everything inlines into the kernel that calls it.  Waves are 64 lanes, workgroups one-dimensional.
// Which sites call which of these, and which stay spelled out because the compiler schedules the kernel around a call
// differently than around the same lines written in place: profiles/epilogue_refactor_codeobj.txt.
#pragma once
#include <hip/hip_runtime.h>

#include "frame_common.hpp"
#include "stack_kernels.h"

namespace nl {

// (wave_sum and lane_rank, which need no StackArgs, are frame_common.hpp's)
// the sum over the wave of an int every lane holds (all 64 lanes active): four DPP steps inside each row of 16 lanes, then the
// four rows through scalar registers -- no LDS crossbar (the __shfl_xor form is 6 ds_bpermute_b32 per value)
__device__ __forceinline__ int wave_sum_dpp(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0xb1, 0xf, 0xf, true);       // quad_perm [1, 0, 3, 2]
    x += __builtin_amdgcn_update_dpp(0, x, 0x4e, 0xf, 0xf, true);       // quad_perm [2, 3, 0, 1]
    x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xf, 0xf, true);      // row_half_mirror
    x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xf, 0xf, true);      // row_mirror
    return (__builtin_amdgcn_readlane(x, 0) + __builtin_amdgcn_readlane(x, 16)) +
           (__builtin_amdgcn_readlane(x, 32) + __builtin_amdgcn_readlane(x, 48));
}

// ---- wave append ----
// The lanes that cannot finish a pixel append it to a hand-over list: the ballot of `flag`, one atomicAdd by lane 0 on
// the list's length where the ballot is not empty, the broadcast of what it returned, each flagged lane's rank among
// the flagged lanes, and the store under slot < capacity (places beyond the capacity are counted, not written: the host
// sees the overflow in the count).  Lanes fill the run in lane order, so the consumer's loads stay coalesced.
// `lane` is the caller's threadIdx.x & 63: every kernel has it at hand, and a second copy of it moves instructions.

template <class T>
__device__ __forceinline__ void wave_append(T *list, unsigned *count, unsigned capacity, bool flag, T value, int lane)
{
    const unsigned long long mask = __ballot(flag);
    if (mask) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(count, (unsigned)__popcll(mask));
        base = __shfl(base, 0, 64);
        const unsigned slot = base + lane_rank(mask, lane);
        if (flag && slot < capacity) list[slot] = value;
    }
}

// ---- clip totals (stack.go:193-198) ----
// Integer atomics into kClipSlots sharded accumulators (integer adds commute: the totals are deterministic), summed by
// reduce_counters_kernel or, under the fused protocol, by fused_collect_slots.
template <class I>
__device__ __forceinline__ unsigned long long *partial_slot(const StackArgs &p, I index)      // (a workgroup's or a wave's index)
{
    return p.partial + 2 * (size_t)(index % kClipSlots);
}
// where a kernel that runs AFTER the dominant one adds its clip counts: the totals (fused protocol, StackArgs::final),
// or a shard
__device__ __forceinline__ unsigned long long *clip_slot(const StackArgs &p, unsigned block)
{
    return p.final ? p.final : partial_slot(p, block);
}
// one thread adds a pair of totals (non-returning atomics; most waves of a clean stack add nothing)
template <class T>
__device__ __forceinline__ void add_clip_totals(unsigned long long *slot, T t_lo, T t_hi)
{
    if (t_lo) atomicAdd(slot + 0, (unsigned long long)t_lo);
    if (t_hi) atomicAdd(slot + 1, (unsigned long long)t_hi);
}

}  // namespace nl
