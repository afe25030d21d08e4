// TEST HARNESS: property test of the basic tier's packed-word child sort
// (raytracer-2025_amd/csrc/rt_sort4.h, the same text the gfx950 kernel's
// visit4_rows compiles).  A visit turns each of a node's four slots into a
// sort word -- the upper 16 bits of the slot's f32 entry distance above the
// child's 16-bit ref code, or SORT4_NONE for an empty slot, a miss or a sphere
// child -- sorts the words with the 5-exchange min / max network, pushes
// words 3, 2, 1 rotated into stack entries and walks word 0 next.  For every
// case:
//   - no real word equals SORT4_NONE, and sort4_least is SORT4_NONE exactly
//     when no slot is hit;
//   - the sorted words are a permutation of the input words;
//   - they are non-decreasing, so the sentinels come last;
//   - no two hit slots whose distances differ in their upper 16 bits are out
//     of order (checked on the f32 distances, not on the words);
//   - every pushed stack entry is bit for bit the entry the (walk word, f32
//     distance) push makes (stack4_word), decodes (stack4_walk_word /
//     stack4_dist, what the pop reads) to the child's ref code and to a
//     positive distance not above the f32 one: the cull stays conservative;
//   - the word walked next is the nearest child's walk word.
// Cases: every arrangement of the four slots over hit and miss, with distances
// drawn from every binade from t_min (f32_down(1e-8)) to 2^60 and +inf (a box
// entered "at infinity" under an unbounded closest t): independent, all in one
// binade, pairs equal in their upper 16 bits, exact ties, t_min itself; ref
// codes over nodes (1 ..= 0x7fff) and list positions (0x8000 ..= 0xffff), the
// extremes included.  Also every pair of neighbouring upper halves: the word
// order is the f32 order.
// Prints "cases pushes violations" and exits 1 on any violation.
// sort4_prop [reps [seed]]
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../raytracer-2025_amd/csrc/rt_sort4.h"

using namespace rtk;

static long bad = 0;
static void fail(const char* what, const bool hit[4], const float e[4], const uint32_t ww[4], const uint32_t w[4]) {
    if (bad < 10) {
        std::printf("VIOLATION %s:", what);
        for (int i = 0; i < 4; ++i)
            std::printf(" [%d %.9g (%08x) %08x]", (int)hit[i], e[i], sort4_f32_bits(e[i]), ww[i]);
        std::printf(" sorted %08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
    }
    ++bad;
}

int main(int argc, char** argv) {
    const int reps = argc > 1 ? std::atoi(argv[1]) : 12;
    std::mt19937_64 rng(argc > 2 ? std::atoll(argv[2]) : 2025);
    auto pick = [&](uint32_t k) { return (uint32_t)(rng() % k); };
    const float tmin_f = f32_down(1e-8);
    const uint32_t tmin_bits = sort4_f32_bits(tmin_f), inf_bits = 0x7f800000u;
    const int e_lo = (int)(tmin_bits >> 23) - 127, e_hi = 60;
    long cases = 0, pushes = 0;

    // the word order is the f32 order: neighbouring upper halves, each with
    // its lowest and highest distance and the extreme ref codes
    for (uint32_t u = tmin_bits >> 16; u < inf_bits >> 16; ++u) {
        const float a = sort4_bits_f32((u << 16) | 0xffffu), b = sort4_bits_f32((u + 1) << 16);
        const uint32_t wa = sort4_word(true, a, 0xffff0000u), wb = sort4_word(true, b, 0x00010000u);
        if (!(a < b) || !(wa < wb) || wa == SORT4_NONE || wb == SORT4_NONE) ++bad;
        ++cases;
    }

    for (int binade = e_lo; binade <= e_hi + 1; ++binade) {  // e_hi + 1: +inf
        for (int pattern = 0; pattern < 6; ++pattern) {
            for (uint32_t mask = 0; mask < 16; ++mask) {
                for (int rep = 0; rep < reps; ++rep) {
                    // a distance of this binade (at least t_min), or of any
                    auto draw = [&](int b) -> float {
                        if (b > e_hi) return sort4_bits_f32(inf_bits);
                        const uint32_t m = pick(4) == 0 ? (pick(2) ? 0u : 0x7fffffu) : pick(1u << 23);
                        const uint32_t bits = ((uint32_t)(b + 127) << 23) | m;
                        return sort4_bits_f32(std::max(bits, tmin_bits));
                    };
                    float e[4];
                    for (int i = 0; i < 4; ++i) e[i] = draw(pattern == 0 ? e_lo + (int)pick(e_hi - e_lo + 1) : binade);
                    if (pattern == 2 || pattern == 3) {  // pairs (or all) equal in their upper 16 bits
                        const int n = pattern == 2 ? 2 : 4, at = pattern == 2 ? (int)pick(3) : 0;
                        for (int i = 1; i < n; ++i)  // (+inf has the one bit pattern)
                            e[at + i] = sort4_bits_f32(std::max(
                                tmin_bits,
                                (sort4_f32_bits(e[at]) & 0xffff0000u) | (binade > e_hi ? 0u : pick(1u << 16))));
                    }
                    if (pattern == 4) {  // exact ties: two, three or four slots
                        const int n = 2 + (int)pick(3);
                        for (int i = 1; i < n; ++i) e[i] = e[0];
                        std::shuffle(e, e + 4, rng);
                    }
                    if (pattern == 5) e[pick(4)] = tmin_f;
                    // distinct children: nodes (index + 1) and list positions
                    // (0x8000 | index) in the walk word's upper half
                    uint32_t ww[4];
                    for (int i = 0; i < 4; ++i) {
                        for (;;) {
                            const uint32_t k = pick(8);
                            const uint32_t code = k == 0 ? 1u : k == 1 ? 0x7fffu : k == 2 ? 0x8000u : k == 3 ? 0xffffu
                                                                                                            : 1u + pick(0xffffu);
                            ww[i] = code << 16;
                            bool dup = false;
                            for (int j = 0; j < i; ++j) dup |= ww[j] == ww[i];
                            if (!dup) break;
                        }
                    }
                    bool hit[4];
                    uint32_t in[4], w[4];
                    int nhit = 0;
                    for (int i = 0; i < 4; ++i) {
                        hit[i] = (mask >> i) & 1u;
                        nhit += hit[i];
                        in[i] = w[i] = sort4_word(hit[i], e[i], ww[i]);
                        if (hit[i] && w[i] == SORT4_NONE) fail("a real word equals the sentinel", hit, e, ww, w);
                        if (!hit[i] && w[i] != SORT4_NONE) fail("a miss is no sentinel", hit, e, ww, w);
                    }
                    ++cases;
                    if ((sort4_least(w) == SORT4_NONE) != (nhit == 0)) fail("least", hit, e, ww, w);
                    sort4(w);
                    uint32_t a[4] = {in[0], in[1], in[2], in[3]}, b[4] = {w[0], w[1], w[2], w[3]};
                    std::sort(a, a + 4);
                    std::sort(b, b + 4);
                    if (!std::equal(a, a + 4, b)) fail("not a permutation", hit, e, ww, w);
                    for (int k = 0; k < 3; ++k)
                        if (w[k] > w[k + 1]) fail("decreasing", hit, e, ww, w);
                    for (int k = 0; k < 4; ++k)
                        if ((w[k] != SORT4_NONE) != (k < nhit)) fail("sentinels not last", hit, e, ww, w);
                    // back to the slots by the ref code
                    int slot[4] = {-1, -1, -1, -1};
                    for (int k = 0; k < nhit; ++k)
                        for (int i = 0; i < 4; ++i)
                            if (hit[i] && (w[k] & 0xffffu) == ww[i] >> 16) slot[k] = i;
                    for (int k = 0; k < nhit; ++k) {
                        if (slot[k] < 0) {
                            fail("ref code lost", hit, e, ww, w);
                            continue;
                        }
                        for (int l = k + 1; l < nhit; ++l) {
                            if (slot[l] < 0) continue;
                            const float ek = e[slot[k]], el = e[slot[l]];
                            if ((sort4_f32_bits(ek) >> 16) != (sort4_f32_bits(el) >> 16) && !(ek < el))
                                fail("distances out of order", hit, e, ww, w);
                        }
                        const int i = slot[k];
                        if (k == 0) {
                            if (sort4_walk_word(w[0]) != ww[i]) fail("walk word", hit, e, ww, w);
                            continue;
                        }
                        const uint32_t entry = sort4_stack_word(w[k]);
                        ++pushes;
                        if (entry != stack4_word(ww[i], e[i])) fail("stack entry format", hit, e, ww, w);
                        if (stack4_walk_word(entry) != ww[i]) fail("stack entry ref code", hit, e, ww, w);
                        const float d = stack4_dist(entry);
                        if (!(d > 0.0f) || !(d <= e[i])) fail("stack entry distance above the f32 one", hit, e, ww, w);
                    }
                    if (nhit == 0 && w[0] != SORT4_NONE) fail("no hit, yet a word to walk", hit, e, ww, w);
                }
            }
        }
    }
    // the list push's entry: never culled (-inf stays -inf)
    {
        const uint32_t entry = stack4_word(0x80010000u, -INFINITY);
        if (stack4_walk_word(entry) != 0x80010000u || !(stack4_dist(entry) == -INFINITY)) ++bad;
        ++cases;
    }
    std::printf("%ld %ld %ld\n", cases, pushes, bad);
    return bad ? 1 : 0;
}
