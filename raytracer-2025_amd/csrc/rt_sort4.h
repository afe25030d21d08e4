// rt_sort4.h -- the basic tier's 4-wide node visit sorts its hit box children
// as packed 32-bit words.
//
// Host and device: the kernel (rt_walk4.h visit4_rows) runs it, and the CPU
// property test (tests/test_sort4_cpu.py, tests/cpp/sort4_prop.cpp) checks the
// same text.
//
// A slot's sort word is the upper 16 bits of its f32 entry distance above the
// child's 16-bit ref code (the upper half of its walk word, rt_stack.h
// bword):
//     sort word  = (bits(entry) & 0xffff0000) | (walk word >> 16)
//  - The entry distance of a hit slot is slab_f's (rt_slab.h): the maximum of
//    the slab entries and t_min > 0, not above the closest t.  So it is
//    positive -- sign bit clear -- and, being an f32 that is no NaN, its bits
//    are at most +inf's 0x7f800000.  Positive f32s order as their bit patterns
//    do as unsigned integers, and so do their upper halves (rounded down: the
//    cut distance is not above the f32 one).  The words therefore sort with
//    one unsigned min and one unsigned max per exchange where (f32 key, ref)
//    pairs take a compare and four selects.
//  - SORT4_NONE = 0xffffffff marks an empty slot, a miss or a sphere child
//    (queued, not walked).  No real word equals it: a real word's upper half
//    is at most 0x7f80.  It is the largest word, so it sorts last.
//  - Children whose distances agree in their upper 16 bits come out in the
//    order of their ref codes.  The closest hit does not depend on the order
//    of the visits, only their number does.
//
// The stack entry (StackB4) is the same two halves the other way round -- the
// ref code above the cut distance -- so a push is one 16-bit rotate of the
// sort word, and the nearest child's walk word one shift.
#pragma once
#include <cstdint>

#include "rt_slab.h"

namespace rtk {

constexpr uint32_t SORT4_NONE = 0xffffffffu;

RT_HD uint32_t sort4_f32_bits(float f) {
    union {
        float f;
        uint32_t u;
    } b{f};
    return b.u;
}
RT_HD float sort4_bits_f32(uint32_t u) {
    union {
        uint32_t u;
        float f;
    } b{u};
    return b.f;
}

// (hi & 0xffff0000) | (lo >> 16): one byte permute on the device
RT_HD uint32_t sort4_halves(uint32_t hi, uint32_t lo) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(hi, lo, 0x07060302u);
#else
    return (hi & 0xffff0000u) | (lo >> 16);
#endif
}

// the sort word of a slot: hit = the slab verdict and "a box child"
RT_HD uint32_t sort4_word(bool hit, float entry, uint32_t walk_word) {
    return hit ? sort4_halves(sort4_f32_bits(entry), walk_word) : SORT4_NONE;
}

RT_HD uint32_t sort4_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
RT_HD uint32_t sort4_max(uint32_t a, uint32_t b) { return a < b ? b : a; }

// the smallest of the four words: SORT4_NONE when no slot is hit
RT_HD uint32_t sort4_least(const uint32_t w[4]) {
    return sort4_min(sort4_min(w[0], w[1]), sort4_min(w[2], w[3]));
}

// the 5-exchange network: w[0] <= w[1] <= w[2] <= w[3] afterwards
RT_HD void sort4(uint32_t w[4]) {
#define RT_SORT4_CX(a, b)                          \
    {                                              \
        const uint32_t lo_ = sort4_min(w[a], w[b]); \
        w[b] = sort4_max(w[a], w[b]);              \
        w[a] = lo_;                                \
    }
    RT_SORT4_CX(0, 1)
    RT_SORT4_CX(2, 3)
    RT_SORT4_CX(0, 2)
    RT_SORT4_CX(1, 3)
    RT_SORT4_CX(1, 2)
#undef RT_SORT4_CX
}

// a sort word's stack entry: the ref code above the cut distance
RT_HD uint32_t sort4_stack_word(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(w, w, 16);
#else
    return (w << 16) | (w >> 16);
#endif
}
// a sort word's walk word (a box child's: the ref code in the upper half)
RT_HD uint32_t sort4_walk_word(uint32_t w) { return w << 16; }

// The stack entry of a walk word and an f32 distance (the list push; the
// visit's pushes are sort4_stack_word of the same halves), and its decoding:
// the walk word and the cut distance, which is not above the pushed one for
// a positive distance (-inf, "never culled", stays -inf).
RT_HD uint32_t stack4_word(uint32_t walk_word, float t) { return sort4_halves(walk_word, sort4_f32_bits(t)); }
RT_HD uint32_t stack4_walk_word(uint32_t e) { return e & 0xffff0000u; }
RT_HD float stack4_dist(uint32_t e) { return sort4_bits_f32(e << 16); }

}  // namespace rtk
