// rt_stack.h -- the per-lane traversal stacks (LDS, with a global overflow),
// the basic tier's walk words and the pops.
#pragma once
#include "rt_builds.h"
#include "rt_kernel.h"
#include "rt_sort4.h"

namespace rtk {

// The per-lane traversal stack: entry k of lane l at stk[k * RT_BLOCK] (the
// pointer is already offset by the lane), {ref, entry distance as f32 rounded
// down} -- one ds_write_b64 / ds_read_b64 per push / pop, 64 distinct banks
// per half-wave.  Entries k >= CAP (deep triangle BVHs) live in the lane's
// column of a global overflow buffer, [k - CAP][lane of the grid], so the LDS
// part stays small enough for 4 blocks per CU.
template <uint32_t CAP>
struct StackT {
    RT_LDS uint2* base;  // explicitly LDS: a select against ovf must not become a flat pointer
    RT_GLOBAL uint2* ovf;
    uint32_t stride;
    // The overflow side moves the entry as one 64-bit word and the LDS side
    // as a uint2: different instructions, so the optimizer cannot merge the
    // two accesses into one through a phi of flat pointers (which also hit a
    // gfx950 code-generation error on an LDS-to-flat cast in the flat tier).
    __device__ __forceinline__ void push(uint32_t sp, uint32_t ref, float t) {
        if (sp >= CAP)
            reinterpret_cast<RT_GLOBAL unsigned long long*>(ovf)[(sp - CAP) * stride] =
                ((unsigned long long)__float_as_uint(t) << 32) | ref;
        else
            base[sp * RT_BLOCK] = make_uint2(ref, __float_as_uint(t));
    }
    __device__ __forceinline__ uint2 at(uint32_t sp) const {
        if (sp >= CAP) {
            const unsigned long long v = reinterpret_cast<const RT_GLOBAL unsigned long long*>(ovf)[(sp - CAP) * stride];
            return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        }
        return base[sp * RT_BLOCK];
    }
};
// Basic tier: 4-B entries -- a list flag and a 15-bit node / list
// index, and the upper 16 bits of the entry distance (a positive f32 cut to
// 16 bits is rounded down: the cull stays conservative; -inf stays -inf).
// The block's stack takes half the LDS; the rest parks walk state.
template <uint32_t CAP, uint32_t BLK>
struct StackB4 {
    RT_LDS uint32_t* base;
    // The basic tier's walk keeps its refs as "words" (bword): a
    // box child's 16-bit stack code in the upper half -- push is one byte
    // permute with the entry distance, pop one mask.  The visit pushes its
    // sorted children as sort words (rt_sort4.h: the same halves the other
    // way round), one 16-bit rotate each.
    __device__ __forceinline__ void push_w(uint32_t sp, uint32_t word, float t) {
        base[sp * BLK] = stack4_word(word, t);
    }
    __device__ __forceinline__ void push_sorted(uint32_t sp, uint32_t sort_word) {
        base[sp * BLK] = sort4_stack_word(sort_word);
    }
    __device__ __forceinline__ uint2 at_w(uint32_t sp) const {
        const uint32_t e = base[sp * BLK];
        return make_uint2(stack4_walk_word(e), __float_as_uint(stack4_dist(e)));
    }
};
// Basic-tier walk words (the 4-wide walk's cur, stack entries and the ref
// row of the block's LDS node copy): 0 = none; a node = (index + 1) << 16;
// a list position = (0x8000 | index) << 16; a sphere = 0x8000 | index (low
// half).  So a box child is word > 0xffff, a sphere child has a nonzero low
// half, and the upper half is the stack entry's ref code as it stands.
// Indices: nodes < 0x7fff (the LDS copy holds 658), lists < 0x8000 and
// spheres < 0x8000 (rt_render.cpp prepare_tier).
__device__ __forceinline__ uint32_t bword(const SceneView& S, uint32_t ref) {
    const uint32_t k = ref_kind(ref), i = ref_idx(S, ref);
    return k == K_BVH ? (i + 1u) << 16 : k == K_LIST ? (0x8000u | i) << 16 : k == K_SPHERE ? (0x8000u | i) : 0u;
}
template <class Stack>
__device__ __forceinline__ uint32_t pop_w(const Stack& stk, uint32_t& sp, float c_f) {
    while (sp > 0) {
        --sp;
        const uint2 e = stk.at_w(sp);
        if (__uint_as_float(e.y) <= c_f) return e.x;
    }
    return 0u;
}
template <int TIER>
struct StackSel {
    using type = StackT<lds_stack_entries(TIER)>;
};
template <>
struct StackSel<TIER_BASIC> {
    using type = StackB4<lds_stack_entries(TIER_BASIC), RT_BLOCK_BASIC>;
};
template <int TIER>
using StackFor = typename StackSel<TIER>::type;

// Pops until an entry whose box can still hold a hit closer than c.
template <class Stack>
__device__ __forceinline__ uint32_t pop(const Stack& stk, uint32_t& sp, uint32_t sp0, float c_f) {
    while (sp > sp0) {
        --sp;
        const uint2 e = stk.at(sp);
        if (__uint_as_float(e.y) <= c_f) return e.x;
    }
    return REF_NONE;
}

template <int TIER>
__device__ __forceinline__ StackFor<TIER> make_stack(RT_LDS uint2* s8, RT_LDS uint32_t* s4, RT_GLOBAL uint2* ovf,
                                                     uint32_t stride) {
    if constexpr (TIER == TIER_BASIC)
        return StackFor<TIER>{s4};
    else
        return StackFor<TIER>{s8, ovf, stride};
}

}  // namespace rtk
