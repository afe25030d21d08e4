// pool_prop.cpp -- the path kernel's work queue on the host (test-only driver of
// raytracer-2025_amd/csrc/rt_queue.h, the text the gfx950 kernels compile):
//
// (a) hand-out: 1..64 simulated waves with random need masks take entries
//     through pool_take / pool_entry from one shared counter until every lane
//     has left.  Every q in [0, queue_total) goes out exactly once, none at or
//     beyond it reaches a lane that stays, every q lies in the pass's
//     [q_lo, q_end), and every lane gets the q -- and the counter every add --
//     that the hand-out gave before the pool moved to scalar registers (kept
//     below as ref_take, with the per-lane guided chunk it sized on every pass);
// (b) decode: queue_entry over all q tiles each item's [0, S) exactly once in
//     the order of the frame plan (rt_plan.h row_parts: whole rows, parts, fine
//     parts), whatever bounds of the pass it is given;
// (c) guided_chunk equals its per-lane predecessor (ref_guided_chunk) on a grid
//     of (pool_end, avail, n) across every region border.
//
//   pool_prop <seed>     prints "<frames> <passes> <entries> <chunk cases>", exit 0 / 1
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../raytracer-2025_amd/csrc/rt_plan.h"
#include "../../raytracer-2025_amd/csrc/rt_queue.h"

using namespace rtk;

// the queue's fields of rt_frame.h Frame, filled as fill_kparams fills them
struct QFrame {
    uint32_t W, rows, S, total_items;
    uint32_t parts, part_len, queue_total, whole_items;
    uint32_t parts2, part_len2, fine_q0, fine_item0;
    uint32_t static_entries, chunk_min, chunk_cap, chunk_min_whole;
    double inv_parts, inv_parts2;
    float inv_guide;
    float S_f, part_len_f, part_len2_f, inv_S_f, inv_part_len_f, inv_part_len2_f;
};

static QFrame make_frame(uint32_t W, uint32_t rows, uint32_t S, uint32_t part_samples, uint32_t fine_samples,
                         uint32_t whole_rows, uint32_t fine_row, uint32_t waves, bool static_pools, uint32_t chunk_min,
                         uint32_t chunk_cap, uint32_t chunk_min_whole) {
    QFrame F{};
    F.W = W, F.rows = rows, F.S = S;
    F.total_items = W * rows * S;
    const uint32_t parts = whole_rows < rows ? plan::row_parts(S, part_samples) : 1u;
    const uint32_t parts2 = fine_row < rows ? plan::row_parts(S, fine_samples) : parts;
    F.parts = parts > 1 ? parts : 1u;
    F.part_len = (S + F.parts - 1) / F.parts;
    F.parts2 = parts2 > 1 ? parts2 : F.parts;
    F.part_len2 = (S + F.parts2 - 1) / F.parts2;
    whole_rows = F.parts > 1 ? std::min(whole_rows, rows) : rows;
    fine_row = fine_row < whole_rows ? whole_rows : std::min(fine_row, rows);
    F.whole_items = W * whole_rows * S;
    F.fine_item0 = W * fine_row * S;
    F.fine_q0 = F.whole_items + (F.fine_item0 - F.whole_items) * F.parts;
    F.queue_total = F.fine_q0 + (F.total_items - F.fine_item0) * F.parts2;
    F.static_entries = static_pools ? 64u * waves : 0u;
    F.chunk_min = chunk_min, F.chunk_cap = chunk_cap, F.chunk_min_whole = chunk_min_whole;
    auto inv_up = [](uint32_t d) { return std::nextafter(1.0 / (double)d, 2.0); };
    F.inv_parts = inv_up(F.parts), F.inv_parts2 = inv_up(F.parts2);
    F.S_f = (float)F.S, F.part_len_f = (float)F.part_len, F.part_len2_f = (float)F.part_len2;
    F.inv_S_f = 1.0f / F.S_f, F.inv_part_len_f = 1.0f / F.part_len_f, F.inv_part_len2_f = 1.0f / F.part_len2_f;
    F.inv_guide = 1.0f / (float)((uint64_t)waves * RT_QUEUE_GUIDE);
    return F;
}

// ---- the reference copies: the queue code as it was, per lane
static void ref_queue_entry(const QFrame& F, uint32_t q, uint32_t& item, uint32_t& s_j, uint32_t& s_end) {
    const bool whole = q < F.whole_items, fine = q >= F.fine_q0;
    const uint32_t qt = whole ? 0u : q - (fine ? F.fine_q0 : F.whole_items);
    const uint32_t np = fine ? F.parts2 : F.parts, pl = fine ? F.part_len2 : F.part_len;
    const uint32_t it = udiv_inv(qt, fine ? F.inv_parts2 : F.inv_parts), part = qt - it * np;
    item = whole ? q : (fine ? F.fine_item0 : F.whole_items) + it;
    s_j = whole ? 0u : part * pl;
    s_end = whole ? F.S : std::min(F.S, s_j + pl);
}
static uint32_t ref_guided_chunk(const QFrame& F, uint32_t pool_end, uint32_t avail, uint32_t n) {
    const uint32_t whole_left = F.whole_items > pool_end ? F.whole_items - pool_end : 0u;
    const uint32_t p0 = std::max(pool_end, F.whole_items), part_left = F.fine_q0 > p0 ? F.fine_q0 - p0 : 0u;
    const uint32_t f0 = std::max(pool_end, F.fine_q0), fine_left = F.queue_total > f0 ? F.queue_total - f0 : 0u;
    const float g = ((float)whole_left * F.S_f + (float)part_left * F.part_len_f + (float)fine_left * F.part_len2_f) *
                    F.inv_guide;
    const float inv_per = whole_left ? F.inv_S_f : (part_left ? F.inv_part_len_f : F.inv_part_len2_f);
    const uint32_t chunk = std::min((uint32_t)(g * inv_per), F.chunk_cap);
    return std::max(std::max(chunk, whole_left ? F.chunk_min_whole : F.chunk_min), avail < n ? n - avail : 0u);
}
struct RefPool {
    uint32_t pool_next, pool_end;
    bool dry;
};
// one pass of n needy lanes: q[rank] of each, adding to `counter` as the leader's atomic did
static void ref_take(RefPool& P, const QFrame& F, uint32_t n, uint32_t& counter, uint32_t* q) {
    const uint32_t avail = P.pool_end - P.pool_next;
    uint32_t fresh = 0;
    const uint32_t chunk = RT_QUEUE_GUIDE ? ref_guided_chunk(F, P.pool_end, avail, n) : (uint32_t)RT_QUEUE_CHUNK;
    if (avail < n) {
        if (!P.dry) {
            fresh = counter + F.static_entries;
            counter += chunk;
            P.dry = fresh + chunk >= F.queue_total;
        } else {
            fresh = F.queue_total;
        }
    }
    const uint32_t old_next = P.pool_next;
    if (avail < n) {
        P.pool_next = fresh + (n - avail);
        P.pool_end = fresh + chunk;
    } else {
        P.pool_next += n;
    }
    for (uint32_t rank = 0; rank < n; ++rank) q[rank] = rank < avail ? old_next + rank : fresh + (rank - avail);
}

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define FAIL(...) (fprintf(stderr, __VA_ARGS__), fprintf(stderr, "\n"), exit(1))

static uint64_t n_passes = 0, n_entries = 0, n_chunks = 0;

// (a)
static void hand_out(const QFrame& F, uint32_t waves, bool static_pools) {
    struct Wave {
        QueuePool pool;
        RefPool ref;
        uint64_t busy, left;  // lanes holding an entry; lanes that have left
    };
    std::vector<Wave> ws(waves);
    for (uint32_t w = 0; w < waves; ++w) {
        ws[w].pool = static_pools ? pool_of_wave(w) : QueuePool{0u, 0u, false};
        ws[w].ref = RefPool{ws[w].pool.next, ws[w].pool.end, false};
        ws[w].busy = ws[w].left = 0;
    }
    std::vector<uint8_t> seen(F.queue_total, 0);
    uint32_t counter = 0, ref_counter = 0, alive = waves;
    const uint32_t finish_odds = 1 + (uint32_t)(rnd() % 7);  // a busy lane finishes a pass with odds 1 / finish_odds
    uint64_t guard = 0;
    while (alive) {
        if (++guard > (uint64_t)64 * (F.queue_total + 64ull * waves + 1024) * 8) FAIL("hand-out does not end");
        Wave& w = ws[rnd() % waves];
        if (w.left == ~0ull) continue;
        // the lanes that need an entry now: every lane not busy, and the busy ones that finish
        uint64_t need = ~w.busy & ~w.left;
        for (uint32_t l = 0; l < 64; ++l)
            if ((w.busy >> l & 1) && rnd() % finish_odds == 0) need |= 1ull << l;
        if (rnd() % 4 == 0) need &= rnd();  // (the kernel's lanes start together; any subset must work)
        const uint32_t n = (uint32_t)__builtin_popcountll(need);
        if (!n) continue;
        ++n_passes;
        uint32_t want[64];
        ref_take(w.ref, F, n, ref_counter, want);
        const QueuePass pass = pool_take(w.pool, F, n, [&](uint32_t chunk) {
            const uint32_t before = counter;
            counter += chunk;
            return before;
        });
        if (counter != ref_counter) FAIL("counter %u, before the change %u", counter, ref_counter);
        if (w.pool.dry != w.ref.dry) FAIL("dry %d, before the change %d", (int)w.pool.dry, (int)w.ref.dry);
        if (!w.pool.dry && (w.pool.next != w.ref.pool_next || w.pool.end != w.ref.pool_end))
            FAIL("pool [%u, %u), before the change [%u, %u)", w.pool.next, w.pool.end, w.ref.pool_next, w.ref.pool_end);
        uint32_t rank = 0;
        for (uint32_t l = 0; l < 64; ++l) {
            if (!(need >> l & 1)) continue;
            const uint32_t q = pool_entry(pass, rank);
            // before the change a dry wave's lanes past the pool got queue_total too; inside a
            // dry wave's last pool the two agree entry for entry
            if (q != want[rank] && !(q >= F.queue_total && want[rank] >= F.queue_total))
                FAIL("lane %u rank %u takes q %u, before the change %u", l, rank, q, want[rank]);
            if (q < pass.q_lo || q >= pass.q_end) FAIL("q %u outside the pass's [%u, %u)", q, pass.q_lo, pass.q_end);
            ++rank;
            if (q >= F.queue_total) {
                w.left |= 1ull << l;
                w.busy &= ~(1ull << l);
            } else {
                if (seen[q]++) FAIL("q %u handed out twice", q);
                ++n_entries;
                w.busy |= 1ull << l;
                // the decode under the pass's bounds is the decode
                uint32_t i0, a0, b0, i1, a1, b1;
                queue_entry(F, q, pass.q_lo, pass.q_end, i0, a0, b0);
                ref_queue_entry(F, q, i1, a1, b1);
                if (i0 != i1 || a0 != a1 || b0 != b1) FAIL("q %u decodes to (%u, %u, %u) under its pass's bounds", q, i0, a0, b0);
            }
        }
        if (w.left == ~0ull) --alive;
    }
    for (uint32_t q = 0; q < F.queue_total; ++q)
        if (seen[q] != 1) FAIL("q %u handed out %u times", q, (unsigned)seen[q]);
}

// (b)
static void decode(const QFrame& F, uint32_t part_samples, uint32_t fine_samples) {
    uint32_t q = 0;
    auto expect = [&](uint32_t item, uint32_t s_j, uint32_t s_end) {
        const uint32_t region_lo = q < F.whole_items ? 0u : q < F.fine_q0 ? F.whole_items : F.fine_q0;
        const uint32_t region_end = q < F.whole_items ? F.whole_items : q < F.fine_q0 ? F.fine_q0 : F.queue_total;
        const uint32_t a = (uint32_t)(rnd() % 70), b = 1 + (uint32_t)(rnd() % 70);
        const uint32_t bounds[5][2] = {{0u, ~0u}, {q, q + 1}, {region_lo, region_end}, {q > a ? q - a : 0u, q + b},
                                       {0u, F.queue_total}};
        for (const auto& bd : bounds) {
            uint32_t i, a0, b0;
            queue_entry(F, q, bd[0], bd[1], i, a0, b0);
            if (i != item || a0 != s_j || b0 != s_end)
                FAIL("q %u in [%u, %u) decodes to item %u [%u, %u), the plan gives item %u [%u, %u)", q, bd[0], bd[1], i, a0,
                     b0, item, s_j, s_end);
        }
        if (s_j >= s_end || s_end > F.S) FAIL("q %u: empty or overlong part [%u, %u)", q, s_j, s_end);
        ++q;
    };
    for (uint32_t item = 0; item < F.total_items; ++item) {
        const bool whole = item < F.whole_items, fine = item >= F.fine_item0;
        const uint32_t np = whole ? 1u : plan::row_parts(F.S, fine ? fine_samples : part_samples);
        if (!whole && np != (fine ? F.parts2 : F.parts)) FAIL("frame set-up: parts");
        const uint32_t len = (F.S + np - 1) / np;
        for (uint32_t p = 0; p < np; ++p) expect(item, p * len, std::min(F.S, (p + 1) * len));
    }
    if (q != F.queue_total) FAIL("the plan enumerates %u entries, queue_total is %u", q, F.queue_total);
}

// (c)
static void chunks(const QFrame& F) {
    std::vector<uint32_t> ends;
    for (uint32_t b : {0u, F.whole_items, F.fine_q0, F.queue_total, F.static_entries})
        for (int d = -2; d <= 2; ++d)
            if ((int64_t)b + d >= 0) ends.push_back(b + d);
    for (int k = 0; k < 24; ++k) ends.push_back((uint32_t)(rnd() % (F.queue_total + 600u)));
    ends.push_back(F.queue_total + 100000u);
    for (uint32_t pool_end : ends)
        for (uint32_t avail : {0u, 1u, 5u, 63u, 64u, 200u, 512u})
            for (uint32_t n : {1u, 2u, 6u, 63u, 64u}) {
                const uint32_t c = guided_chunk(F, pool_end, avail, n), r = ref_guided_chunk(F, pool_end, avail, n);
                if (c != r) FAIL("guided_chunk(%u, %u, %u) = %u, per lane %u", pool_end, avail, n, c, r);
                if (avail < n && c < n - avail) FAIL("guided_chunk(%u, %u, %u) = %u: short of the wave's need", pool_end, avail, n, c);
                ++n_chunks;
            }
}

int main(int argc, char** argv) {
    rng_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    struct Shape {
        uint32_t W, rows, S, part_samples, fine_samples, whole_rows, fine_row;
    };
    const Shape shapes[] = {
        {4, 2, 1, 4, 1, 2, 2},      // 8 entries: fewer than a wave's lanes
        {8, 8, 1, 4, 1, 8, 8},      // exactly 64
        {13, 5, 1, 4, 1, 5, 5},     // 65
        {13, 5, 1, 4, 1, 3, 4},     // S = 1 cannot split: the tail rows stay whole
        {16, 9, 4, 2, 1, 9, 9},     // whole rows only
        {16, 9, 4, 2, 1, 5, 9},     // parts, no fine parts
        {16, 9, 4, 2, 1, 5, 8},     // parts and fine parts
        {16, 9, 4, 2, 1, 0, 0},     // fine parts only
        {16, 9, 4, 2, 1, 0, 9},     // parts only
        {3, 7, 4, 2, 1, 2, 2},      // whole rows, then fine parts
        {16, 9, 22, 4, 1, 9, 9},    // 3 168 whole rows: above one chunk
        {16, 9, 22, 4, 1, 5, 8},    // the headline's split (22 samples: 6 parts, 22 fine parts)
        {5, 3, 22, 4, 1, 1, 2},
        {1, 1, 22, 4, 1, 0, 0},     // one pixel in fine parts: 484 entries of one sample
    };
    uint64_t n_frames = 0;
    for (const Shape& sh : shapes)
        for (uint32_t waves : {1u, 2u, 3u, 7u, 16u, 64u})
            for (int static_pools = 0; static_pools < 2; ++static_pools) {
                // the launcher's chunk settings (floor 64, cap 512) and small ones, so that small queues take many chunks
                const uint32_t mins[3] = {64u, 1u, 7u}, caps[3] = {512u, 16u, 40u}, min_whole[3] = {0u, 0u, 9u};
                const int k = (int)(n_frames % 3);
                const QFrame F = make_frame(sh.W, sh.rows, sh.S, sh.part_samples, sh.fine_samples, sh.whole_rows,
                                            sh.fine_row, waves, static_pools != 0, mins[k], caps[k], min_whole[k]);
                if (waves == 1 && !static_pools) decode(F, sh.part_samples, sh.fine_samples);
                if (waves <= 3) chunks(F);
                hand_out(F, waves, static_pools != 0);
                ++n_frames;
            }
    printf("%llu %llu %llu %llu\n", (unsigned long long)n_frames, (unsigned long long)n_passes,
           (unsigned long long)n_entries, (unsigned long long)n_chunks);
    return 0;
}
