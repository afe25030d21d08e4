// rt_walk4.h -- the visits of a 4-wide node (every BVH tier) and the basic
// tier's walk step over them (trace4_step).
#pragma once
#include "rt_walk.h"
#include "rt_sort4.h"

namespace rtk {

// Every BVH tier walks 4-wide nodes (rth::bvh4_convert).  Basic tier: sphere
// children go through the slab test of their own f32 box (rt_slab.h
// sphere_box_f) into a per-lane LDS queue of exact tests (visit4_rows).  Mesh
// and full tiers: every child boxed (visit4_boxes), for the walk and the
// medium boundary walks.  (rt_sphere_filter.h is not called by the path
// kernels: only rt_walk_selftest runs it.)
#ifndef RT_PEND_CAP
#define RT_PEND_CAP 8  // queued sphere tests per lane (LDS, 2 B each: sphere index < 65536)
#endif

// ------------------------------------------------------------------ basic tier: sphere rounds
#ifndef RT_DEFER_THRESH
#define RT_DEFER_THRESH 48  // lanes with a queued sphere that trigger a sphere round
#endif
// ... or 3/4 of the lanes still in the walk, when fewer than 64 are; and any
// one of them when at most RT_DEFER_THIN are: a wave thinned out at the end
// of a launch tests its queued spheres at once instead of walking on with an
// unbounded walk (a ray trapped in a glass sphere queues the sphere it starts
// on at every bounce: its origin is on the surface, inside the sphere's box).
// Measured within noise on the whole frame and on the 1/8 shard:
// the slow last waves of the lane trace were the exit atomics' (the kernel's
// end), not this.
#ifndef RT_DEFER_THIN
#define RT_DEFER_THIN 16
#endif

// ------------------------------------------------------------------ basic tier: 4-wide BVH
// One visit of a DNode4: four slab tests; a sphere child whose box is hit is
// queued for its exact test (the lane's LDS queue, pq[k * RT_BLOCK_BASIC]);
// the hit box children are sorted by entry distance, the nearest is walked
// next and the others pushed farthest first.  (Until round 7 a sphere child
// went through the f32 sphere filter of rt_sphere_filter.h instead: about 30
// VALU instructions a slot beside the slab's 19, and eleven per-ray registers;
// the box admits more rays -- 1.88 exact tests a ray on C2 instead of 1.49 --
// and gives the walk no early bound -- 5.32 node visits a ray instead of 5.01
// -- yet C2 is 3.5 % faster: profiles/r07/ab_boxed_spheres_c2_128spp.json.)
// The sort runs on packed words (rt_sort4.h): the upper half of the entry
// distance above the child's 16-bit ref code, min / max per exchange, and a
// 16-bit rotate makes the stack entry -- where (f32 key, ref) pairs took a
// compare and four selects per exchange and a byte permute per push.
struct Node4Rows {
    float4 lx, ly, lz, hx, hy, hz, rq;
};
// The node rows from the block's LDS copy: the launcher gives the basic tier
// only worlds whose whole 4-wide tree fits it (NODE_LDS_CAP nodes: about 900
// spheres; larger sphere worlds run the mesh tier).  A per-wave
// fallback to global reads for larger trees cost 88 B/lane of scratch at the
// 128-VGPR budget.
__device__ __forceinline__ Node4Rows load_node4(const RT_LDS float4* nl, uint32_t idx) {
    const RT_LDS float4* np = nl + idx * 7u;
    return Node4Rows{np[0], np[1], np[2], np[3], np[4], np[5], np[6]};
}
// The same node with each axis' rows in the order the lane's ray meets them
// (Trav::so): the near row of axis k is row k + s and its far row 3 + k - s,
// with s = 0 where 1/d > 0 and 3 otherwise -- an add on the node's address
// per row, the row's constant in the read's offset field, and still seven
// ds_read_b128.  The slab test then needs no min / max to pair an axis' two
// plane distances (rt_slab.h slab_sorted_f): 6 VALU fewer a slot.
struct Node4Sorted {
    float4 nx, ny, nz, fx, fy, fz, rq;
};
__device__ __forceinline__ Node4Sorted load_node4_sorted(const RT_LDS float4* nl, uint32_t idx, const uint32_t so[3]) {
    const RT_LDS char* np = (const RT_LDS char*)(nl + idx * 7u);
    auto row = [](const RT_LDS char* p, int r) { return ((const RT_LDS float4*)p)[r]; };
    return Node4Sorted{row(np + so[0], 0), row(np + so[1], 1), row(np + so[2], 2), row(np - so[0], 3),
                       row(np - so[1], 4), row(np - so[2], 5), row(np, 6)};
}
// visit4 on node rows already loaded; the ref row holds walk words (bword).
// The check build also gets the rows as stored (raw) and the unsorted ray
// (rf), runs slab_f beside every slab_sorted_f and reports a differing
// verdict, or a differing entry on a hit, through check_fail as index `node`
// under the marker kind K_CHECK_SLAB: every render on the check library holds the two tests' agreement
// as the GPU compiles them.
template <class Stack>
__device__ __forceinline__ uint32_t visit4_rows(const SceneView& S, const Node4Sorted& nr, const RaySF& sf,
                                                float tmin_f, float c_f, Stack& stk, uint32_t& sp,
                                                RT_LDS uint16_t* pq, uint32_t& pn, const Node4Rows& raw,
                                                const RayF& rf, uint32_t node) {
    const float4 nx = nr.nx, ny = nr.ny, nz = nr.nz, fx = nr.fx, fy = nr.fy, fz = nr.fz, rq = nr.rq;
    const float NX[4] = {nx.x, nx.y, nx.z, nx.w}, NY[4] = {ny.x, ny.y, ny.z, ny.w}, NZ[4] = {nz.x, nz.y, nz.z, nz.w};
    const float FX[4] = {fx.x, fx.y, fx.z, fx.w}, FY[4] = {fy.x, fy.y, fy.z, fy.w}, FZ[4] = {fz.x, fz.y, fz.z, fz.w};
    const uint32_t R[4] = {__float_as_uint(rq.x), __float_as_uint(rq.y), __float_as_uint(rq.z), __float_as_uint(rq.w)};
#ifdef RT_CHECK
    const float LX[4] = {raw.lx.x, raw.lx.y, raw.lx.z, raw.lx.w}, LY[4] = {raw.ly.x, raw.ly.y, raw.ly.z, raw.ly.w};
    const float LZ[4] = {raw.lz.x, raw.lz.y, raw.lz.z, raw.lz.w}, HX[4] = {raw.hx.x, raw.hx.y, raw.hx.z, raw.hx.w};
    const float HY[4] = {raw.hy.x, raw.hy.y, raw.hy.z, raw.hy.w}, HZ[4] = {raw.hz.x, raw.hz.y, raw.hz.z, raw.hz.w};
#endif
    uint32_t w[4];
    // per slot, one slab test when some lane has a child there: a sphere
    // child's row holds its own box (rth::bvh4_convert), and a hit queues it
    // for the exact test where a box child's hit gets its sort word
    // (rt_sort4.h: the upper half of the entry distance above the ref code).
    // The queue takes the walk word's low half as it stands -- trace4_step
    // masks the sphere flag off where it reads the index.  The flatten puts
    // a node's empty slots last.
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        // a child is a box (word > 0xffff, low half zero) or a sphere (upper
        // half zero): the sphere flag comes from the two compares the slot
        // needs anyway, as a mask operation
        const bool any = R[i] != 0u, box = R[i] > 0xffffu, sph = any && !box;
        w[i] = SORT4_NONE;
        if (__ballot(any)) {
            const float nr3[3] = {NX[i], NY[i], NZ[i]}, fr3[3] = {FX[i], FY[i], FZ[i]};
            float e;
            const bool h = slab_sorted_f(nr3, fr3, sf, tmin_f, c_f, e);
#ifdef RT_CHECK
            {
                const float lo[3] = {LX[i], LY[i], LZ[i]}, hi[3] = {HX[i], HY[i], HZ[i]};
                float e0;
                const bool h0 = slab_f(lo, hi, rf, tmin_f, c_f, e0);
                if (any && (h0 != h || (h && __float_as_uint(e0) != __float_as_uint(e)))) check_fail(make_ref(K_CHECK_SLAB, node));
            }
#endif
            // The queue store is unconditional and only the count is not: a
            // lane that queues nothing writes above its queue's top, into an
            // entry nothing reads before the next push overwrites it.  That
            // entry exists: a lane visits with pn <= RT_PEND_CAP - 4
            // (trace4_step's ROOM) and slot i has added at most i, so the
            // index is at most RT_PEND_CAP - 1.  An address, a store and a
            // select-and-add where the store under its own lane mask took an
            // instruction and two mask operations more (C2 -1.0 %,
            // profiles/r08/ab_packed_sort_variants_c2_128spp.json).
            pq[pn * RT_BLOCK_BASIC] = (uint16_t)R[i];
            pn += h && sph ? 1u : 0u;
            w[i] = sort4_word(h && box, e, R[i]);
        }
    }
    // no lane of the wave hit a box child (nodes of spheres only, or every
    // box missed): nothing to sort or push (C2 -0.65 %, A/B at 128 spp, 5
    // reps, RMSE 0; a two-slot network when no lane has a box in slots 0 and
    // 1 was +1.9 %)
    if (!__ballot(sort4_least(w) != SORT4_NONE)) return 0u;
    sort4(w);
    if (w[3] != SORT4_NONE) stk.push_sorted(sp++, w[3]);
    if (w[2] != SORT4_NONE) stk.push_sorted(sp++, w[2]);
    if (w[1] != SORT4_NONE) stk.push_sorted(sp++, w[1]);
    return w[0] != SORT4_NONE ? sort4_walk_word(w[0]) : 0u;
}

// One visit of a DNode4 whose children all carry boxes (mesh tier): four slab
// tests, the hit children sorted by entry distance, the nearest walked next
// and the others pushed farthest first -- primitives included, so a triangle
// is tested (planar_t) when the walk reaches it, in distance order.
template <class Stack>
__device__ __forceinline__ uint32_t visit4_core(const float LX[4], const float LY[4], const float LZ[4],
                                                const float HX[4], const float HY[4], const float HZ[4],
                                                const uint32_t R[4], const RayF& rf, float tmin_f, float c_f,
                                                Stack& stk, uint32_t& sp);
template <class Stack>
__device__ __forceinline__ uint32_t visit4_boxes_rows(const float4 lx, const float4 ly, const float4 lz,
                                                      const float4 hx, const float4 hy, const float4 hz,
                                                      const float4 rq, const RayF& rf, float tmin_f, float c_f,
                                                      Stack& stk, uint32_t& sp) {
    const float LX[4] = {lx.x, lx.y, lx.z, lx.w}, LY[4] = {ly.x, ly.y, ly.z, ly.w}, LZ[4] = {lz.x, lz.y, lz.z, lz.w};
    const float HX[4] = {hx.x, hx.y, hx.z, hx.w}, HY[4] = {hy.x, hy.y, hy.z, hy.w}, HZ[4] = {hz.x, hz.y, hz.z, hz.w};
    const uint32_t R[4] = {__float_as_uint(rq.x), __float_as_uint(rq.y), __float_as_uint(rq.z), __float_as_uint(rq.w)};
    return visit4_core(LX, LY, LZ, HX, HY, HZ, R, rf, tmin_f, c_f, stk, sp);
}
template <class Stack>
__device__ __forceinline__ uint32_t visit4_boxes(const SceneView& S, uint32_t idx, const RayF& rf, float tmin_f,
                                                 float c_f, Stack& stk, uint32_t& sp) {
    const RT_GLOBAL float4* np = reinterpret_cast<const RT_GLOBAL float4*>(S.nodes4 + idx);
    return visit4_boxes_rows(np[0], np[1], np[2], np[3], np[4], np[5], np[6], rf, tmin_f, c_f, stk, sp);
}
template <class Stack>
__device__ __forceinline__ uint32_t visit4_core(const float LX[4], const float LY[4], const float LZ[4],
                                                const float HX[4], const float HY[4], const float HZ[4],
                                                const uint32_t R[4], const RayF& rf, float tmin_f, float c_f,
                                                Stack& stk, uint32_t& sp) {
    constexpr float INF = __builtin_huge_valf();
    float key[4];
    uint32_t ref[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float lo[3] = {LX[i], LY[i], LZ[i]}, hi[3] = {HX[i], HY[i], HZ[i]};
        float e;
        const bool h = slab_f(lo, hi, rf, tmin_f, c_f, e) && R[i] != REF_NONE;
        key[i] = h ? e : INF;
        ref[i] = R[i];
    }
    auto cs = [&](int a, int b) {
        const bool sw = key[b] < key[a];
        const float ka = key[a], kb = key[b];
        const uint32_t ra = ref[a], rb = ref[b];
        key[a] = sw ? kb : ka;
        key[b] = sw ? ka : kb;
        ref[a] = sw ? rb : ra;
        ref[b] = sw ? ra : rb;
    };
    cs(0, 1);
    cs(2, 3);
    cs(0, 2);
    cs(1, 3);
    cs(1, 2);
    if (key[3] < INF) stk.push(sp++, ref[3], key[3]);
    if (key[2] < INF) stk.push(sp++, ref[2], key[2]);
    if (key[1] < INF) stk.push(sp++, ref[1], key[1]);
    return key[0] < INF ? ref[0] : REF_NONE;
}

// world.hit for the basic tier over 4-wide nodes, one wave iteration per call:
// a node round (f32 only) for lanes with room in their queue, then a sphere
// round -- each lane with a queued sphere tests one exactly in f64
// (sphere.rs:77-108) -- when 48 lanes have one queued or none can walk on.  A
// lane whose queue is full waits for that before walking on.  Returns false
// when the lane's walk and queue are both done; same closest hit as
// trace_step's walk (A/B renders: RMSE 0).
template <class Stack>
__device__ __forceinline__ bool trace4_step(const SceneView& S, const Ray& r, Trav<TIER_BASIC>& T, Stack& stk,
                                            RT_LDS uint16_t* pq, const RT_LDS float4* nl, Diag& dg) {
    constexpr double tmin = 1e-8;
    const float tmin_f = f32_down(tmin);
    // a visit queues at most 4 (one per slot), and a lane visits only with
    // pn <= ROOM: the lane's LDS queue never overflows.  (A lane that waits
    // for its round with any sphere queued, ROOM = 0, so that the bound comes
    // before the next node: C2 +16.6 %, profiles/r07/ab_boxed_spheres_c2_128spp.json)
    static_assert(RT_PEND_CAP >= 4, "a visit may queue 4 spheres: the lane's LDS queue must hold them");
    constexpr uint32_t ROOM = RT_PEND_CAP - 4;
    RT_DIAG_ONLY(if (__lane_id() == (uint32_t)(__ffsll((long long)__ballot(true)) - 1)) ++dg.wave_trace_iters;)
    uint32_t pn = T.pn;
    // The sphere round is decided on the state before this step's node
    // round and its sphere load issued first, ahead of the node's seven LDS
    // reads; its f64 test comes after the node visit, by when the load has
    // landed.
    const bool has = T.cur != 0u || T.sp > 0;  // a word to walk, now or on the stack
    const bool can = has && pn <= ROOM;
    // (the AND of two ballots, each a compare into a scalar pair: the ballot
    // of the AND goes through a 0 / 1 vector register and a second compare)
    const unsigned long long mh0 = __ballot(has);
    const unsigned long long mw0 = mh0 & __ballot(pn <= ROOM);
    const unsigned long long mp0 = __ballot(pn > 0);
    // The lanes in the walk are those with a word to walk or a sphere queued
    // (what the last step returned true for, or a walk just begun): the
    // batch loop calls the step with every lane of the wave, and a lane whose
    // walk is over, or that has no path, holds the empty state -- it cannot
    // walk, has no round, reads entry 0 like every lane without one, and
    // returns false.  The count as a 32-bit scalar the compiler cannot see
    // through: it otherwise widens the compare below to 64 bits, which only
    // the vector unit has.
    uint32_t in_walk = (uint32_t)__popcll(mh0 | mp0);
    asm("" : "+s"(in_walk));
    const uint32_t thresh =
        in_walk <= RT_DEFER_THIN ? 1u : min((uint32_t)RT_DEFER_THRESH, (in_walk * 3u + 3u) / 4u);
    const bool round = (mw0 == 0 || (uint32_t)__popcll(mp0) >= thresh) && pn > 0;
#ifdef RT_DIAG
    if (mw0 == 0 && __lane_id() == (uint32_t)(__ffsll((long long)__ballot(true)) - 1)) {
        ++dg.pure_rounds;
        dg.pure_lanes += (unsigned long long)__popcll(mp0);
    }
    if (mw0 == 0) {  // the most spheres any lane of the wave still has queued
        uint32_t mx = 0;
        for (uint32_t k = 1; k <= RT_PEND_CAP; ++k) mx += __ballot(pn >= k) != 0ull ? 1u : 0u;
        if (__lane_id() == (uint32_t)(__ffsll((long long)__ballot(true)) - 1)) dg.pure_max_pn += mx;
    }
#endif
    // the loads are unconditional (a lane without a round / a node reads
    // entry 0, cache-hot) so that no branch stands between them and their
    // waits: the sphere test then waits for its own load only
    const uint32_t top = pn > 0 ? pn - 1 : 0;
    const uint32_t sidx = pq[top * RT_BLOCK_BASIC] & 0x7fffu;  // queued with the walk word's sphere flag
    pn -= round ? 1u : 0u;
    const double4 s4 = S.spheres[round ? sidx : 0u];
    uint32_t cur = REF_NONE;
    if (can) {
        RT_DIAG_ONLY(++dg.lane_trace_iters;)
#ifdef RT_DIAG
        if (T.cur == 0u) {
            const uint32_t sp_before = T.sp;
            T.cur = pop_w(stk, T.sp, T.cl.c_f);
            ++dg.pops;
            dg.pop_reads += sp_before - T.sp;
        }
#else
        if (T.cur == 0u) T.cur = pop_w(stk, T.sp, T.cl.c_f);
#endif
        cur = T.cur;
        T.cur = 0u;
    }
    // cur is a walk word (bword): a node, a list position or a sphere
    const uint32_t r16 = cur >> 16;
    const bool node = r16 - 1u < 0x7fffu;  // 1 ..= 0x7fff
    const Node4Sorted rows = load_node4_sorted(nl - 7, node ? r16 : 1u, T.so);
#ifdef RT_CHECK
    const Node4Rows raw = load_node4(nl - 7, node ? r16 : 1u);
#else
    const Node4Rows raw{};  // read by the check build only
#endif

    if (__ballot(!node && cur != 0u)) {  // lists, standalone spheres (none in C2)
        if (r16 >= 0x8000u) {  // a list position
            const uint32_t li = r16 & 0x7fffu;
            const uint32_t child = S.list_children[li];
            if (child != REF_NONE) {
                if (S.list_children[li + 1] != REF_NONE) stk.push_w(T.sp++, (0x8000u | (li + 1)) << 16, NO_CULL);
                T.cur = bword(S, child);
            }
        } else if (r16 == 0u && cur != 0u) {  // a sphere element of a list: queued for its exact test
            // (the lane's own word decides: the block is entered on the
            // wave's ballot, and a lane at a node, or with no word at all --
            // waiting for its round, or holding the empty state -- queues
            // nothing here.  Until round 10 such a lane queued its word's
            // low half, sphere 0: a test more that changed no hit, and for a
            // lane at a node a fifth entry ahead of the visit's four.)
            pq[pn * RT_BLOCK_BASIC] = (uint16_t)cur;
            ++pn;
        }
    }
    if (node) {
        RT_ISA_MARK("walk_visit");
        RT_DIAG_ONLY(++dg.node_visits;)
        T.cur = visit4_rows(S, rows, T.sf, tmin_f, T.cl.c_f, stk, T.sp, pq, pn, raw, T.rf, r16 - 1u);
    }
    // the sphere round's f64 test after the node visit: the visit's LDS rows
    // arrive before the sphere's global load, and the test then finds it
    // there (C2 -0.2 %, profiles/r05/ab_round_late_c2_128spp.json; the
    // visit culls against the closest t before this test, which only makes
    // it cull less, never wrongly)
    if (round) {  // sphere round (sphere.rs:77-108)
        RT_ISA_MARK("walk_sphere");
        RT_DIAG_ONLY(++dg.sphere_tests;)
        double t;
        RT_DIAG_ONLY(if (s4.w > 100.0) ++dg.big_tests;)
        if (sphere_t_inv(d3(s4.x, s4.y, s4.z), s4.w, r, T.a, T.inva, tmin, T.cl.c, t)) {
            RT_DIAG_ONLY(if (s4.w > 100.0) ++dg.big_hits;)
            T.cl.lower(t);
            T.found = true;
            T.hit.t = t;
            T.hit.ref = make_ref(K_SPHERE, sidx);
        }
    }
    RT_ISA_MARK("walk_tail");
    T.pn = pn;
    return T.cur != 0u || T.sp > 0 || pn > 0;
}

// Basic tier: the block's copy of the world's 4-wide nodes (at most CAP: the
// launcher gives the tier no larger tree), the ref rows as walk words (bword);
// ends on the block's barrier.  A macro, unlike walk_lds (rt_walk.h): as a
// __forceinline__ function template (node_lds as a pointer or as an array
// reference) the loop compiles differently in rt_path_kernel<TIER_BASIC> --
// the LDS store's address runs from 0x12000 up, not from 0x12008 with an
// offset of -8, the kernel is two instructions shorter (7 496 lines of
// llvm-objdump -d for 7 498) and every later address moves -- and the path
// kernels' code objects were to stay byte for byte what they were when the
// hit kernels came in.  walk_lds leaves all five identical.  The next change
// that re-measures the basic tier anyway can make this a function.
#define RT_COPY_NODES_LDS(S, node_lds, CAP, BLK)                                                      \
    do {                                                                                              \
        const uint32_t n_lds = min((S).n_nodes4, (CAP)); /* == n_nodes4 (launcher) */                 \
        const RT_GLOBAL float4* src = reinterpret_cast<const RT_GLOBAL float4*>((S).nodes4);          \
        for (uint32_t k = threadIdx.x; k < n_lds * 7u; k += (BLK)) {                                  \
            float4 v = src[k];                                                                        \
            if (k % 7u == 6u) { /* the ref row: walk words (bword) */                                 \
                v.x = __uint_as_float(bword((S), __float_as_uint(v.x)));                              \
                v.y = __uint_as_float(bword((S), __float_as_uint(v.y)));                              \
                v.z = __uint_as_float(bword((S), __float_as_uint(v.z)));                              \
                v.w = __uint_as_float(bword((S), __float_as_uint(v.w)));                              \
            }                                                                                         \
            (node_lds)[k] = v;                                                                        \
        }                                                                                             \
        __syncthreads();                                                                              \
    } while (0)

}  // namespace rtk
