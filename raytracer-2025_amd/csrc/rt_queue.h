// rt_queue.h -- the path kernel's work queue as the wave sees it: the pool of
// queue entries a wave holds (QueuePool), the pass that hands entries out of
// it and takes the next chunk from the frame's counter (pool_take), the
// chunk's size (guided_chunk) and the decode of an entry into its stratum row
// and samples (queue_entry).  Plain integer and f32 arithmetic, templates over
// the frame type (rt_frame.h Frame: the fields named here), so that the
// same text compiles for the host: tests/cpp/pool_prop.cpp drives simulated
// waves through it.  How a frame splits into entries is rt_plan.h's business.
//
// Everything in pool_take and guided_chunk is wave-uniform: the pool derives
// from the wave's index, the popcount of a ballot, one lane's atomic result
// and launch parameters.  The compiler cannot see that through the loop that
// carries the pool, so every value stored into it goes through
// v_readfirstlane (q_uniform); the pass is then scalar code and `avail < n`
// a scalar branch.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_Q_HD __host__ __device__ __forceinline__
#else
#define RT_Q_HD inline
#endif

#ifndef RT_QUEUE_CHUNK
// most entries a wave takes per queue atomic, with chunks shrinking as
// left / (waves x RT_QUEUE_GUIDE): 512 / 16 against 256 / 8 -- half the
// counter's atomics early, smaller pools late -- C2 186.3 -> 185.0 ms frame
// and 1/8 shard 24.8 -> 24.4, C4 188.6 -> 186.2 and 29.8 -> 26.7, C3 +-0.5 %
// (A/B, 2 interleaved reps each; 512 at guide 8: C2 frame -1.1 % but shard
// +11 %; 512 / 32 and 1024 / 32: C2 shard +4-5 %)
#define RT_QUEUE_CHUNK 512
#endif
#ifndef RT_QUEUE_CHUNK_MESH
// the mesh tier's cap, a knob: its rounds are long (a dependent global load
// per walk step) and a large pool can outlive the queue by milliseconds, but
// smaller caps cost the whole frame in counter contention (at guide 8, cap
// 128: C4 frame +2 %, 1/8 shard 30.0 -> 27.3 ms; 64: +6 %, 27.2 ms)
#define RT_QUEUE_CHUNK_MESH RT_QUEUE_CHUNK
#endif
#ifndef RT_QUEUE_GUIDE
#define RT_QUEUE_GUIDE 16  // guided chunks: left / (waves * GUIDE), 0 = fixed RT_QUEUE_CHUNK
#endif

namespace rtk {

RT_Q_HD uint32_t q_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
RT_Q_HD uint32_t q_max(uint32_t a, uint32_t b) { return a < b ? b : a; }
// a wave-uniform value, told to the compiler (on the host: the value)
RT_Q_HD uint32_t q_uniform(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
#else
    return x;
#endif
}

// n / d for n < 2^32, d < 2^20, from inv = 1/d rounded up: n * inv is at least
// the quotient's integer part when d divides n (a representable product,
// rounded to nearest, cannot fall below it) and below the next integer
// otherwise (the excess n * 2^-52 / d stays under 1/d): three f64 / convert
// instructions instead of a ~25-instruction integer division expansion.
RT_Q_HD uint32_t udiv_inv(uint32_t n, double inv) { return (uint32_t)((double)n * inv); }

// Queue entry q -> its stratum-row item and samples [s_j, s_end) (Frame:
// whole rows, then parts, then the fine parts of the frame's last rows).
// The frame's fields are read first and the regions' values selected
// afterwards: written as `fine ? F.a : F.b` the select lands on the address,
// and the field becomes a per-lane load from the launch parameters where a
// scalar load serves the whole wave.
//
// [q_lo, q_end) bounds the entries of the wave's pass (QueuePass; any q, any
// bounds that hold q: 0 and ~0u know nothing).  Nearly every pass lies in one
// region, and then which region is a scalar compare: a pass of whole rows
// has nothing to decode, and a pass of parts picks its region's constants by
// scalar select and divides by a scalar.  Only a pass across a region's
// border selects per lane.  All three give the same item and samples.
template <class FrameT>
RT_Q_HD void queue_entry(const FrameT& F, uint32_t q, uint32_t q_lo, uint32_t q_end, uint32_t& item, uint32_t& s_j,
                         uint32_t& s_end) {
    const uint32_t whole_items = F.whole_items, fine_q0 = F.fine_q0, fine_item0 = F.fine_item0, S = F.S;
    if (q_end <= whole_items) {
        item = q;
        s_j = 0u;
        s_end = S;
        return;
    }
    const uint32_t parts = F.parts, parts2 = F.parts2, part_len = F.part_len, part_len2 = F.part_len2;
    const double inv_parts = F.inv_parts, inv_parts2 = F.inv_parts2;
    if (q_lo >= fine_q0 || (q_lo >= whole_items && q_end <= fine_q0)) {
        const bool fine = q_lo >= fine_q0;
        const uint32_t np = fine ? parts2 : parts, pl = fine ? part_len2 : part_len;
        const uint32_t qt = q - (fine ? fine_q0 : whole_items);
        const uint32_t it = udiv_inv(qt, fine ? inv_parts2 : inv_parts), part = qt - it * np;
        item = (fine ? fine_item0 : whole_items) + it;
        s_j = part * pl;
        s_end = q_min(S, s_j + pl);
        return;
    }
    const bool whole = q < whole_items, fine = q >= fine_q0;
    const uint32_t qt = whole ? 0u : q - (fine ? fine_q0 : whole_items);  // (udiv_inv wants n < 2^32 in range)
    const uint32_t np = fine ? parts2 : parts, pl = fine ? part_len2 : part_len;
    const uint32_t it = udiv_inv(qt, fine ? inv_parts2 : inv_parts), part = qt - it * np;
    item = whole ? q : (fine ? fine_item0 : whole_items) + it;
    s_j = whole ? 0u : part * pl;
    s_end = whole ? S : q_min(S, s_j + pl);
}

// The guided chunk of a wave whose pool ends at pool_end: about 1/GUIDE of
// the samples left (as last seen) per wave of the grid, in the entries of
// the region the next pool starts in; never below what the wave's lanes need
// now (n lanes, avail entries in the pool), nor below Frame::chunk_min.  Near
// the end a wave takes only what its lanes need: a pool held by a slow wave
// (deep glass paths) is work the idle waves cannot take
// (scripts/lane_trace.py).  (The chunk in the entries it takes: a pool of
// whole rows taken as the tail starts is no larger in samples than the tail's
// pools -- it would outlast them.)  The f32 expression and its order are the
// chunk: the order entries go out in, and with it the frame's bits, hold only
// while every build evaluates it as written.
template <class FrameT>
RT_Q_HD uint32_t guided_chunk(const FrameT& F, uint32_t pool_end, uint32_t avail, uint32_t n) {
    const uint32_t whole_items = F.whole_items, fine_q0 = F.fine_q0, queue_total = F.queue_total;
    const uint32_t whole_left = whole_items > pool_end ? whole_items - pool_end : 0u;
    const uint32_t p0 = q_max(pool_end, whole_items), part_left = fine_q0 > p0 ? fine_q0 - p0 : 0u;
    const uint32_t f0 = q_max(pool_end, fine_q0), fine_left = queue_total > f0 ? queue_total - f0 : 0u;
    const float g = ((float)whole_left * F.S_f + (float)part_left * F.part_len_f + (float)fine_left * F.part_len2_f) *
                    F.inv_guide;
    const float inv_S_f = F.inv_S_f, inv_part_len_f = F.inv_part_len_f, inv_part_len2_f = F.inv_part_len2_f;
    const float inv_per = whole_left ? inv_S_f : (part_left ? inv_part_len_f : inv_part_len2_f);
    const uint32_t chunk = q_min((uint32_t)(g * inv_per), F.chunk_cap);
    const uint32_t chunk_min_whole = F.chunk_min_whole, chunk_min = F.chunk_min;
    return q_max(q_max(chunk, whole_left ? chunk_min_whole : chunk_min), avail < n ? n - avail : 0u);
}

// The queue entries a wave holds: [next, end).  Wave w of the grid starts
// with the 64 entries [64 w, 64 w + 64) -- no atomic at launch: 4096 waves
// taking their first chunk from one counter at once waited up to 2.9 ms for
// it (scripts/lone_wave.py) -- and the counter hands out entries from
// Frame::static_entries on.  `dry`: an atomic of this wave has passed the end
// of the queue, so none will hand out entries any more -- lanes that need
// one leave without another atomic (the drain's waves waited ~70 us a round
// on the counter the whole grid hammered).
struct QueuePool {
    uint32_t next, end;
    bool dry;
};
RT_Q_HD QueuePool pool_of_wave(uint32_t wave) {
    const uint32_t first = q_uniform(wave * 64u);
    return QueuePool{first, first + 64u, false};
}

// One pass of the hand-out: the wave's n needy lanes (n >= 1) take entries in
// rank order, first what the pool holds (avail, from old_next on), the rest
// from the start of a chunk taken now (fresh); pool_entry is the lane's.
// fetch_add(chunk) adds chunk to the frame's counter and returns its value
// before.  The chunk is sized only here, where one is taken: a pool holds up
// to 512 entries and a pass hands out a few, so nearly every pass skips it.
// A dry wave takes none: the lanes past the pool get queue_total, the
// entry no lane runs.  [q_lo, q_end) holds every entry the pass hands out
// (queue_entry's bounds).
struct QueuePass {
    uint32_t old_next, avail, fresh, q_lo, q_end;
};
template <class FrameT, class FetchAdd>
RT_Q_HD QueuePass pool_take(QueuePool& P, const FrameT& F, uint32_t n, FetchAdd&& fetch_add) {
    QueuePass r{P.next, P.end - P.next, 0u, P.next, P.next + n};
    uint32_t chunk = 0u;
    if (r.avail < n) {
        const uint32_t queue_total = F.queue_total, short_by = n - r.avail;
        chunk = short_by;
        if (!P.dry) {
            chunk = q_uniform(RT_QUEUE_GUIDE ? guided_chunk(F, P.end, r.avail, n) : (uint32_t)RT_QUEUE_CHUNK);
            r.fresh = q_uniform(fetch_add(chunk) + F.static_entries);
            P.dry = q_uniform(r.fresh + chunk >= queue_total);
        } else {
            r.fresh = queue_total;
        }
        r.q_lo = q_min(r.old_next, r.fresh);
        r.q_end = q_max(P.end, r.fresh + short_by);
        P.next = r.fresh + short_by;
        P.end = r.fresh + chunk;
    } else {
        P.next = r.old_next + n;
    }
    return r;
}
RT_Q_HD uint32_t pool_entry(const QueuePass& r, uint32_t rank) {
    return rank < r.avail ? r.old_next + rank : r.fresh + (rank - r.avail);
}

}  // namespace rtk
