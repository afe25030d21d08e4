// rt_kernel_path.hip -- the path kernel (rt_path_kernel) and the host entry
// points of its tiers.  The product library compiles this unit once per tier
// (-DRT_TIER=N, each object with its own code-generation flags:
// raytracer-2025_amd/Makefile); with RT_TIER undefined it instantiates all
// six tiers and the basic tier's wide variant (the whole build,
// rt_kernel.hip).  The trace, check and diag builds' readers live here, with
// the kernels that write what they read.
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_slab.h"
#include "rt_primary.h"
#include "rt_plan.h"
#include "rt_queue.h"
#include "rt_path_entry.h"
// the device code, in the order of rt_kernel.hip's map
#include "rt_builds.h"
#include "rt_frame.h"
#include "rt_texture.h"
#include "rt_geom.h"
#include "rt_stack.h"
#include "rt_walk.h"
#include "rt_walk4.h"
#include "rt_record.h"
#include "rt_lights.h"
#include "rt_shade.h"

namespace rtk {

// ------------------------------------------------------------------ the kernel
#ifndef RT_BASIC_WAVES
#define RT_BASIC_WAVES 4  // waves per SIMD the basic tier is register-allocated for
#endif
#ifndef RT_FULL_WAVES
#define RT_FULL_WAVES 2  // full tier (C5): 2 waves without spills, shading in batches of 56 (below)
#endif
#ifndef RT_FLAT_WAVES
#define RT_FLAT_WAVES 3  // FULL_FLAT
#endif
// Lanes of a wave that must have finished their walk before it shades (64 =
// all).  Trace-heavy worlds (deep triangle BVHs) gain from shading in batches;
// for C2 the shading divergence of small batches costs more than the walks
// gain (A/B in DESIGN.md).
#ifndef RT_SHADE_BATCH_BASIC
// basic tier over a tree of at most NODE_LDS_CAP_BATCH nodes (C1 / C2: 241):
// shading in 56-lane batches, the carried-over walks parked in LDS (32 KiB
// taken from the node copy).  Round 5, with the shared-draws loop: C2 -2.3 %
// kernel time against whole-wave shading (A/B at 128 spp, RMSE 0; round 2's
// loop had measured +1.7 %).  Larger trees (up to NODE_LDS_CAP) run the
// whole-wave variant of the tier (rt_path_kernel<TIER_BASIC, true>).
#define RT_SHADE_BATCH_BASIC 56
#endif
#ifndef RT_SHADE_BATCH_MESH
#define RT_SHADE_BATCH_MESH 48
#endif
#ifndef RT_SHADE_BATCH_FULL
// C5 walks are uneven (37 % lane efficiency with whole-wave shading): at 2
// waves/SIMD the 256-VGPR budget holds the walk state across a shading batch
// without spills, C5 -12 % against 3 waves / whole-wave shading; at 3 waves
// batches spill 372 B/lane and cost +65 %
#define RT_SHADE_BATCH_FULL 56
#endif
#ifndef RT_SHADE_BATCH_FLAT
#define RT_SHADE_BATCH_FLAT 64
#endif
#ifndef RT_MESH_WAVES
#define RT_MESH_WAVES 4  // beats 2 waves (164.7 vs 263.8 ms, C4 64 spp) and 3 / 5 waves (+16 % / +12 %)
#endif

// WIDE (basic tier only): the variant for trees of NODE_LDS_CAP_BATCH +
// 1 .. NODE_LDS_CAP nodes -- the whole LDS node copy, whole-wave shading, no
// park area.
template <int TIER, bool WIDE = false>
__global__ void __launch_bounds__(TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK, TIER == TIER_FULL_FLAT ? RT_FLAT_WAVES : tier_full_bvh(TIER) ? RT_FULL_WAVES : (TIER == TIER_MESH ? RT_MESH_WAVES : RT_BASIC_WAVES))
    rt_path_kernel(const KParams* __restrict__ P) {
    static_assert(!WIDE || TIER == TIER_BASIC, "the wide variant is the basic tier's");
    constexpr int BASIC_BATCH = WIDE ? 64 : RT_SHADE_BATCH_BASIC;
    constexpr uint32_t NODE_CAP = WIDE ? NODE_LDS_CAP : NODE_LDS_CAP_BATCH;
    // The params block is read-only for the launch: scalar loads, hoisted.
    const SceneView S = P->S;
    const Frame& F = P->F;
    uint32_t* queue = P->queue;
    constexpr int STACK = lds_stack_entries(TIER);
    constexpr uint32_t BLK = TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    constexpr bool B4 = TIER == TIER_BASIC;
    // The lane arena (all tiers but the basic one): one uint2 row per lane and
    // row, RT_BLOCK apart -- the stack's rows, then (full tiers) the media
    // queue's (MedQ), then (full-flat tier) the parked path state's -- so
    // that every per-lane LDS access is one base address (threadIdx.x * 8)
    // plus a constant in the instruction's offset field, not a base VGPR per
    // array held across the path loop
    constexpr bool LDS_STATE = TIER == TIER_FULL_FLAT;
    constexpr bool PARK_RAY = LDS_STATE;  // + the world ray (7 doubles)
    constexpr uint32_t R_MED = lane_rows_med<TIER>();
    constexpr uint32_t R_PST = R_MED + (tier_full(TIER) ? 2u * RT_MEDIA_CAP : 0u);
    constexpr uint32_t R_PIT = R_PST + (LDS_STATE ? (PARK_RAY ? 16u : 9u) : 0u);
    constexpr uint32_t R_END = R_PIT + (LDS_STATE ? 2u : 0u);
    __shared__ uint2 lane_lds[B4 ? 1 : R_END * BLK];
    __shared__ uint32_t stack4_lds[B4 ? STACK * BLK : 1];
    __shared__ uint16_t pend_lds[B4 ? RT_PEND_CAP * BLK : 1];
    const WalkLds<TIER> wl = walk_lds<TIER>(lane_lds, stack4_lds, pend_lds, P->stack_ovf);
    RT_LDS uint2* const lrow = wl.lrow;
    const MedQ med = wl.med;
    RT_LDS uint16_t* pq = wl.pq;
    StackFor<TIER> stk = wl.stk;
    // Basic tier with shading batches: the walk state of a lane whose walk
    // carries over a shading round is parked here across it (RT_PARK_WORDS
    // words: cur, sp | pn | found, c, c_f, hit t, hit ref), so that the
    // shading code does not hold it in registers.
    constexpr bool PARK = (TIER == TIER_BASIC && BASIC_BATCH < 64) ||
                          (TIER == TIER_MESH && RT_SHADE_BATCH_MESH < 64);
    __shared__ __attribute__((aligned(16))) uint32_t park_lds[PARK ? RT_PARK_WORDS * BLK : 1];
    RT_LDS uint32_t* pk = (RT_LDS uint32_t*)(park_lds + threadIdx.x);
    RT_LDS uint2* pk2 = (RT_LDS uint2*)park_lds + threadIdx.x;  // basic tier: 8-byte rows (trace_park2)
    // Basic tier: the block's copy of the world's 4-wide nodes (the whole tree:
    // 241 nodes for C1/C2), read by every node visit instead of global memory.
    __shared__ float4 node_lds[B4 ? NODE_CAP * 7 : 1];
    if constexpr (B4) RT_COPY_NODES_LDS(S, node_lds, NODE_CAP, BLK);
    if constexpr (tier_full_bvh(TIER)) {
        if (S.n_perlin > 0) {
            const RT_GLOBAL float4* src = reinterpret_cast<const RT_GLOBAL float4*>(S.perlin);
            RT_LDS float4* dst = (RT_LDS float4*)&g_perlin_lds;
            for (uint32_t k = threadIdx.x; k < sizeof(DPerlin) / 16; k += BLK) dst[k] = src[k];
            __syncthreads();
        }
    }
    // Full-flat tier: the path state the walk never reads (beta, L, acc, the
    // item's fields) is parked in LDS across the walk, so that its registers
    // are free there instead of spilled to scratch around it.
    RT_LDS double* const pst = (RT_LDS double*)(lrow + R_PST * BLK);
    RT_LDS uint2* const pit = lrow + R_PIT * BLK;
    // ... and the queue entry's running sum and part-sum slot stay there for
    // the whole entry (pst rows 6-8, pit row 1 .y): read at the sample's end
    // only, they hold no registers through the shading code
    constexpr bool ACC_LDS = LDS_STATE;

    Rng rng;
    rng.k0 = F.key0;
    rng.k1 = F.key1;
    // the lane's queue entry: stratum row s_i of pixel rng.pixel (= py * W +
    // px), samples s_j ..< s_end (sie = s_i | s_end << 16: S < 2^16),
    // partial-sum slot `slot` -- few registers across the path loop
    uint32_t slot = 0, s_j = 0, sie = 0;
    bool need = true;
    bool in_path = false;
    // defined from the start: the basic tier's walk-field set-up reads it for
    // lanes without a path too (values never used; no indeterminate read)
    Ray ray{};
    D3 beta = d3(1, 1, 1), L = d3(0, 0, 0), acc = d3(0, 0, 0);
    uint32_t vertex = 0;
    uint32_t n_rays = 0, n_panics = 0;

    // wave-uniform, in scalar registers: the queue entries this wave holds
    // (rt_queue.h)
    QueuePool pool = pool_of_wave(blockIdx.x * (BLK / 64) + threadIdx.x / 64);
    Diag dg;
    Trav<TIER> T;
    bool walking = false;
#ifdef RT_WAVE_TRACE
    const uint32_t trace_lane = blockIdx.x * BLK + threadIdx.x;
    const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long trace_c0 = __builtin_amdgcn_s_memtime();
    uint32_t trace_items = 0, trace_q = 0, trace_rays = 0, trace_steps = 0, trace_steps_q = 0;
    // the wave's queue atomics: count and the ticks from issue to return
    // (wave-uniform; every lane holds the wave's value)
    unsigned long long trace_atomic_ticks = 0, trace_atomic_first = 0;
    uint32_t trace_atomics = 0;
    RayHist hist;
    hist.t0 = trace_t0;  // (an s_memrealtime: one value per wave)
    unsigned long long trace_tq = trace_t0;
#endif
    // ---- refill: the lanes that need a queue entry take one (false: the
    // queue is done and this lane leaves the loop).  Both loops below run it,
    // in uniform control flow: the pool is the wave's.
    auto refill = [&]() -> bool {
        // wave-aggregated dequeue of stratum rows.  The wave takes a chunk of
        // entries per atomic into its pool and hands them to its lanes in
        // rank order: one contended atomic per chunk, not one per main-loop
        // iteration (every iteration some lane of the wave needs work).
        const unsigned long long mask = __ballot(need);
        if (mask) {
            // the lane's rank among the needy lanes (the leader: rank 0 with
            // need); the leader's atomic result is read with v_readlane -- no
            // lane id held across the loop, no ds_bpermute
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                            __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
            const QueuePass pass = pool_take(pool, F, (uint32_t)__popcll(mask), [&](uint32_t chunk) -> uint32_t {
                const uint32_t leader = __ffsll((long long)mask) - 1;
#ifdef RT_WAVE_TRACE
                const unsigned long long ta = __builtin_amdgcn_s_memrealtime();
#endif
                uint32_t fresh = 0;
                if (need && rank == 0) fresh = atomicAdd(queue, chunk);
                fresh = __builtin_amdgcn_readlane(fresh, leader);
#ifdef RT_WAVE_TRACE
                {
                    const unsigned long long tb = __builtin_amdgcn_s_memrealtime();
                    trace_atomic_ticks += tb - ta;
                    if (trace_atomics++ == 0) trace_atomic_first = tb - trace_t0;
                }
#endif
                return fresh;
            });
            if (need) {
                const uint32_t q = pool_entry(pass, rank);
                if (q >= F.queue_total) return false;
                need = false;
#ifdef RT_WAVE_TRACE
                ++trace_items;
                trace_q = q;
                trace_rays = n_rays;
                trace_steps_q = trace_steps;
                trace_tq = __builtin_amdgcn_s_memrealtime();
#endif
                uint32_t item, s_end;
                if constexpr (B4)
                    queue_entry(F, q, pass.q_lo, pass.q_end, item, s_j, s_end);
                else
                    queue_entry(F, q, 0u, ~0u, item, s_j, s_end);
                if constexpr (ACC_LDS)  // the entry's sum lives in LDS (flat tier)
                    pst[6 * RT_BLOCK] = 0.0, pst[7 * RT_BLOCK] = 0.0, pst[8 * RT_BLOCK] = 0.0;
                else
                    acc = d3(0, 0, 0);
                const uint32_t pl = udiv_inv(item, F.inv_S), s_i = item - pl * F.S;
                sie = s_i | (s_end << 16);
                if constexpr (ACC_LDS)
                    pit[BLK].y = q;
                else
                    slot = q;
                const uint32_t prow = udiv_inv(pl, F.inv_W);
                rng.pixel = (F.row_offset + prow * F.row_stride) * F.W + (pl - prow * F.W);
            }
        }
        return true;
    };
    // ---- the end of a lane's sample (camera.rs:193's sum, in s_j order): its
    // radiance joins the entry's sum; the entry's last sample writes the sum
    auto finish_sample = [&]() {
        if (isnan(L.x) || isnan(L.y) || isnan(L.z)) {  // camera.rs:323
            ++n_panics;
            L = d3(0, 0, 0);
        }
        acc = acc + L;
        ++s_j;
        if (s_j == (sie >> 16)) {
            double* dst = P->partial + (uint64_t)slot * 3;
            dst[0] = acc.x;
            dst[1] = acc.y;
            dst[2] = acc.z;
            need = true;
        }
    };
    if constexpr (TIER == TIER_BASIC) {
        // Basic / mesh tiers: a lane's iteration is walk -> (miss: the sample
        // ends) -> refill -> draws -> shade or a new sample's camera ray, so
        // that the one Philox block and sincos of the iteration's Draws serve
        // both (struct Draws).  A lane whose path ends in shading (depth,
        // panic, no scatter) starts its next sample one iteration later.
        // That is the wide variant's iteration; the batch variant's is walk
        // -> (miss) -> refill -> a new sample's camera draws, camera ray and
        // candidate tests -> the vertex draws -> shade (PRIM, below).
        bool no_path = true;  // the lane starts a sample at its next post-walk stage
        constexpr int BATCH = BASIC_BATCH;
        // Batch variant: a lane that starts a sample resolves its camera ray
        // in the post-walk pass, by the exact sphere test on its pixel's
        // candidates (rt_primary.h; the launch's table, P->cand), and shades
        // a hit in the same pass with the walked hits.  The closest hit does
        // not depend on the order of the tests, so the hit is the walk's.  A
        // camera ray that hits nothing (`pmiss`) sits out the next walk phase
        // and ends its sample in that iteration's miss stage; a pixel with
        // more candidates than the table holds sends its rays through the walk.
        constexpr bool PRIM = !WIDE;
        bool pmiss = false;
        // ---- Camera::get_ray (camera.rs:247-273), vertex 0, from the iteration's draws
        auto camera_ray = [&](const Draws& Dr) {
            const uint32_t s_i = sie & 0xFFFFu, py = udiv_inv(rng.pixel, F.inv_W), px = rng.pixel - py * F.W;
            double xi0 = Dr.xi0, xi1 = Dr.xi1;
            D3 origin = F.center;
            if (F.defocus) {  // vec3.rs:63-69: theta = 2 pi Dr.xi0, r = sqrt(Dr.xi1)
                rng.pair(0u, 0u, xi0, xi1);
                const double rr = k_sqrt(Dr.xi1);
                origin = (F.center + ((rr * Dr.cs) * F.disk_u)) + ((rr * Dr.sn) * F.disk_v);
            }
            const double ox = (((double)s_i + xi0) * F.recip_sqrt_spp) - 0.5;
            const double oy = (((double)s_j + xi1) * F.recip_sqrt_spp) - 0.5;
            const D3 ps = (F.pixel00 + (((double)px + ox) * F.du)) + (((double)py + oy) * F.dv);
            ray.o = origin;
            ray.d = ps - origin;
            ray.time = 0.0;  // read only by moving spheres (full tiers): its draw is skipped
            beta = d3(1, 1, 1);
            L = d3(0, 0, 0);
            vertex = 1;
            no_path = false;
        };
        for (;;) {
            RT_DIAG_ONLY(const unsigned long long t_loop0 = __builtin_amdgcn_s_memtime(); ++dg.main_iters;)
            RT_ISA_MARK("fields");
#ifdef RT_WAVE_TRACE
            hist.add(__ballot(!no_path && !walking && !pmiss));
#endif
            if constexpr (TIER == TIER_BASIC && PARK) {
                // a new walk and a walk carried over the last shading round
                // make the same ray-derived fields: once, for both (as two
                // branches the wave ran that code twice in most rounds: C2
                // -0.7 %, profiles/r05/ab_shared_rayfields_c2_128spp.json).
                // A lane with no path (it starts its sample after this walk
                // phase) sets up the walk state too, which it does not walk:
                // the state is then defined on every path into the walk, so
                // that the compiler need not keep the last walk's values live
                // through the shading code (C2 -1.6 %: 28 B/lane of scratch
                // -> none, 128 -> 124 VGPRs; ab_define_t_c2_128spp.json).
                // Its state is the empty one -- no word to walk, nothing
                // queued: the walk loop below steps every lane of the wave
                trace_ray_fields(ray, T);
                if (!walking) {
                    T.cl.c = __builtin_huge_val();
                    T.cl.c_f = __builtin_huge_valf();
                    T.sp = 0;
                    T.found = false;
                    T.pn = 0;
                    T.nxf = 0;
                    T.hit.nxf = 0;
                    T.nmed = 0;
                    // (a camera ray that missed every candidate has no walk either)
                    const bool begin = !no_path && !pmiss;
                    T.cur = begin ? bword(S, S.world_root) : 0u;
                    if (begin) {
                        rng.begin(vertex);
                        ++n_rays;
                        walking = true;
                    }
                } else {
                    trace_unpark_state2(T, pk2);
                }
            } else if (!no_path && !walking) {  // the whole-wave variant: every walk ends in the walk phase
                rng.begin(vertex);
                ++n_rays;
                trace_begin<TIER>(S, ray, T);
                walking = true;
            }
            RT_DIAG_ONLY(const unsigned long long t_b0 = __builtin_amdgcn_s_memtime(); dg.cyc_refill += t_b0 - t_loop0;)
            RT_ISA_MARK("walk");
            auto step = [&]() -> bool {
                return trace4_step(S, ray, T, stk, pq, (const RT_LDS float4*)node_lds, dg);
            };
            if constexpr (BATCH >= 64) {
#ifdef RT_WAVE_TRACE
                while (walking) walking = step(), ++trace_steps;
#else
                while (walking) walking = step();
#endif
            } else {
                // Every lane of the wave takes the step, in uniform control
                // flow: a lane that is not walking holds the empty state, on
                // which a step does nothing and returns false.  The step's
                // verdict is then a compare of every lane, and its ballot the
                // compare's own mask -- under `if (walking)` the verdict was
                // merged into the lanes' mask, and the ballot went through a
                // 0 / 1 vector register and a second compare at every step
                // (C2 -2.0 %, profiles/r10/ab_walk_rounds_c2_128spp.json).
                const unsigned long long active = __ballot(true);
                if (__ballot(walking))
                    for (;;) {
                        walking = step();
                        const unsigned long long w = __ballot(walking);
                        uint32_t done = (uint32_t)__popcll(active & ~w);
                        asm("" : "+s"(done));  // (a 32-bit scalar compare: see trace4_step's in_walk)
                        if (w == 0 || done >= (uint32_t)BATCH) break;
                    }
            }
            RT_DIAG_ONLY(const unsigned long long t_b1 = __builtin_amdgcn_s_memtime(); dg.cyc_trace += t_b1 - t_b0;)
            // a walk that carries over this shading round is parked;
            // the lane skips the rest of the iteration but for the refill,
            // which every lane of the wave runs: the queue pool (QueuePool:
            // next, end, dry) is wave-uniform state and must be updated in
            // uniform control flow, or a parked lane would keep a stale copy
            RT_ISA_MARK("park");
            const bool carry = BATCH < 64 && walking;
            if constexpr (PARK) {
                if (carry) trace_park2(T, pk2);
            }
            // ---- this lane's walk is over, or it has no path
            bool cam = no_path;
            if (!carry && !no_path && !T.found) {  // a miss: Environment::value, and the sample ends
                RT_ISA_MARK("miss");
                bool panic = false;
                shade<TIER>(S, ray, beta, L, rng, false, T.hit, panic);
                if (panic) ++n_panics;
                finish_sample();
                cam = true;
                if constexpr (PRIM) pmiss = false;
            }
            RT_DIAG_ONLY(const unsigned long long t_m = __builtin_amdgcn_s_memtime(); dg.cyc_miss += t_m - t_b1;)
            RT_ISA_MARK("refill");
            if (!refill()) break;
            RT_DIAG_ONLY(const unsigned long long t_q = __builtin_amdgcn_s_memtime(); dg.cyc_queue += t_q - t_m;)
            if (carry) continue;
            if constexpr (PRIM) {
                // ---- a new sample: its own camera draws (vertex 0: the pixel
                // offsets at slots 0 and 1; with a lens, theta and r at slots 2
                // and 3 and the sincos), the camera ray, and the exact test
                // of the pixel's candidates, which fills T.hit / T.found as
                // the walk would have
                RT_ISA_MARK("camera");
                bool hit = !cam;  // the lanes the shading stages run for: walked hits, and primary hits
                if (cam) {
                    rng.sample = (sie & 0xFFFFu) * F.S + s_j;
                    Draws Dc;
                    rng.pair(0u, F.defocus ? 1u : 0u, Dc.xi0, Dc.xi1);
                    Dc.sn = 0.0, Dc.cs = 0.0;
                    if (F.defocus) k_sincos_2pi(Dc.xi0, &Dc.sn, &Dc.cs);
                    camera_ray(Dc);
                    const uint32_t py = udiv_inv(rng.pixel, F.inv_W), px = rng.pixel - py * F.W;
                    const uint32_t prow = udiv_inv(py - F.row_offset, P->inv_stride);
                    const RT_GLOBAL uint4* const tab = P->cand;
                    uint4 w = make_uint4(PRIMARY_WALK, 0u, 0u, 0u);
                    if (tab) w = tab[(uint64_t)prow * F.W + px];
                    if ((w.x & 0xffffu) != PRIMARY_WALK) {
                        rng.begin(vertex);  // the walk's start, without the walk
                        ++n_rays;
                        const double a = len2(ray.d), inva = 1.0 / a;
                        Closest cl;
                        cl.c = __builtin_huge_val();
                        bool found = false;
                        uint32_t href = 0;
                        for (;;) {
                            const uint32_t idx = w.x & 0xffffu;
                            if (idx >= PRIMARY_NONE) break;
                            // the next slot; the mark shifted in ends a full row
                            w.x = __builtin_amdgcn_alignbit(w.y, w.x, 16u);
                            w.y = __builtin_amdgcn_alignbit(w.z, w.y, 16u);
                            w.z = __builtin_amdgcn_alignbit(w.w, w.z, 16u);
                            w.w = (w.w >> 16) | (PRIMARY_WALK << 16);
                            const double4 s4 = S.spheres[idx];
                            RT_DIAG_ONLY(++dg.prim_tests;)
                            double t;
                            // (sphere.rs:77-108, the sphere rounds' own test: a
                            // root equal to the closest one takes the hit, as there)
                            if (sphere_t_inv(d3(s4.x, s4.y, s4.z), s4.w, ray, a, inva, 1e-8, cl.c, t)) {
                                cl.c = t;
                                found = true;
                                href = make_ref(K_SPHERE, idx);
                            }
                        }
#ifdef RT_CHECK
                        {  // check build: the walk of the same ray must find the same hit
                            Trav<TIER_BASIC> Tc;
                            trace_begin<TIER_BASIC>(S, ray, Tc);
                            bool wk = true;
                            while (wk) wk = trace4_step(S, ray, Tc, stk, pq, (const RT_LDS float4*)node_lds, dg);
                            if (Tc.found != found ||
                                (found && __double_as_longlong(Tc.hit.t) != __double_as_longlong(cl.c)))
                                check_fail(make_ref(K_CHECK_PRIMARY, rng.pixel & 0x0fffffffu));
                        }
#endif
                        RT_DIAG_ONLY(++dg.prim_rays;)
                        T.found = found;
                        T.hit.t = cl.c;
                        T.hit.ref = href;
                        T.hit.nxf = 0;
                        pmiss = !found;
                        hit = found;
                    }
                }
                RT_DIAG_ONLY(const unsigned long long t_c = __builtin_amdgcn_s_memtime(); dg.cyc_refill += t_c - t_b1;
                             dg.cyc_camera += t_c - t_q;)
                if (hit) {
                    // the vertex's draws (slots 0 and 1) and one ray_color
                    // level (camera.rs:275-325) at depth max_depth - vertex + 1
                    RT_ISA_MARK("draws");
                    Draws Dr;
                    rng.pair(vertex, 0u, Dr.xi0, Dr.xi1);
                    k_sincos_2pi(Dr.xi0, &Dr.sn, &Dr.cs);
                    RT_DIAG_ONLY(const unsigned long long t_d = __builtin_amdgcn_s_memtime(); dg.cyc_refill += t_d - t_c;
                                 dg.cyc_draws += t_d - t_c;)
                    RT_ISA_MARK("shade");
                    rng.begin(vertex);
                    rng.slot = 2;  // slots 0 and 1 are Dr
                    bool panic = false;
                    bool end_path = shade_hit_basic(S, ray, beta, T.hit, panic, Dr);
                    if (panic) {
                        ++n_panics;
                        end_path = true;
                    }
                    if (!end_path) {
                        ++vertex;
                        if (vertex > F.max_depth) end_path = true;  // depth == 0 -> BLACK (camera.rs:282-284)
                    }
                    if (end_path) {
                        finish_sample();
                        no_path = true;
                    }
                    RT_DIAG_ONLY(dg.cyc_shade += __builtin_amdgcn_s_memtime() - t_d;)
                }
                continue;
            }
            // the iteration's draws: a hit's (vertex, slots 0 and 1) or a new
            // sample's camera draws (vertex 0: theta and r of the defocus disk
            // at slots 2 and 3, else the pixel offsets at slots 0 and 1)
            RT_ISA_MARK("draws");
            if (cam) rng.sample = (sie & 0xFFFFu) * F.S + s_j;
            Draws Dr;
            rng.pair(cam ? 0u : vertex, (cam && F.defocus) ? 1u : 0u, Dr.xi0, Dr.xi1);
            k_sincos_2pi(Dr.xi0, &Dr.sn, &Dr.cs);
            RT_DIAG_ONLY(const unsigned long long t_d = __builtin_amdgcn_s_memtime(); dg.cyc_refill += t_d - t_b1;
                         dg.cyc_draws += t_d - t_q;)
            if (!cam) {
                RT_ISA_MARK("shade");
                // ---- one ray_color level (camera.rs:275-325) at depth max_depth - vertex + 1
                rng.begin(vertex);
                rng.slot = 2;  // slots 0 and 1 are Dr
                bool panic = false;
                bool end_path;
                if constexpr (!WIDE)  // (the wide variant spills 76 B/lane with the merged stages)
                    end_path = shade_hit_basic(S, ray, beta, T.hit, panic, Dr);
                else
                    end_path = shade<TIER>(S, ray, beta, L, rng, true, T.hit, panic, Dr);
                if (panic) {
                    ++n_panics;
                    end_path = true;
                }
                if (!end_path) {
                    ++vertex;
                    if (vertex > F.max_depth) end_path = true;  // depth == 0 -> BLACK (camera.rs:282-284)
                }
                if (end_path) {
                    finish_sample();
                    no_path = true;
                }
                RT_DIAG_ONLY(dg.cyc_shade += __builtin_amdgcn_s_memtime() - t_d;)
            } else {
                RT_ISA_MARK("camera");
                camera_ray(Dr);
                RT_DIAG_ONLY(dg.cyc_refill += __builtin_amdgcn_s_memtime() - t_d;)
            }
        }
    } else {
    for (;;) {
        RT_DIAG_ONLY(const unsigned long long t_loop0 = __builtin_amdgcn_s_memtime(); ++dg.main_iters;)
        if (!refill()) break;
        if (!in_path) {
            // ---- Camera::get_ray (camera.rs:247-273), vertex 0
            const uint32_t s_i = sie & 0xFFFFu, py = udiv_inv(rng.pixel, F.inv_W), px = rng.pixel - py * F.W;
            rng.sample = s_i * F.S + s_j;
            rng.begin(0);
            uint32_t ovf = 0;
            const double xi0 = rng.next(ovf), xi1 = rng.next(ovf);
            const double ox = (((double)s_i + xi0) * F.recip_sqrt_spp) - 0.5;
            const double oy = (((double)s_j + xi1) * F.recip_sqrt_spp) - 0.5;
            const D3 ps = (F.pixel00 + (((double)px + ox) * F.du)) + (((double)py + oy) * F.dv);
            D3 origin = F.center;
            if (F.defocus) {
                const double xt = rng.next(ovf);  // theta = 0.0 + (2.0 * PI - 0.0) * xt = 2.0 * PI * xt (vec3.rs:63-69)
                const double rr = k_sqrt(rng.next(ovf));
                double sn, cs;
                k_sincos_2pi(xt, &sn, &cs);
                origin = (F.center + ((rr * cs) * F.disk_u)) + ((rr * sn) * F.disk_v);
            }
            ray.o = origin;
            ray.d = ps - origin;
            // the ray's time (vertex 0's last draw) is read only by moving
            // spheres, which only the full tiers hold: the basic and mesh
            // tiers skip its Philox block (no other draw depends on it)
            ray.time = tier_full(TIER) ? rng.next(ovf) : 0.0;
            beta = d3(1, 1, 1);
            L = d3(0, 0, 0);
            vertex = 1;
            in_path = true;
        }

        // ---- one ray_color level (camera.rs:275-325) at depth max_depth - vertex + 1:
        // world.hit as a resumable walk.  The wave walks until RT_SHADE_BATCH of its
        // lanes have finished (or none walks any more); those are shaded and get
        // their next ray while the unfinished walks carry over to the next round,
        // so short walks do not idle behind the longest one of the wave.
#ifdef RT_WAVE_TRACE
        hist.add(__ballot(!walking));
#endif
        if (!walking) {
            rng.begin(vertex);
            ++n_rays;
            trace_begin<TIER>(S, ray, T);
            walking = true;
        } else if constexpr (PARK) {
            trace_unpark(ray, T, pk);  // a walk carried over the last shading round
        }
        RT_DIAG_ONLY(const unsigned long long t_b0 = __builtin_amdgcn_s_memtime(); dg.cyc_refill += t_b0 - t_loop0;)
        constexpr int BATCH = TIER == TIER_MESH ? RT_SHADE_BATCH_MESH
                            : TIER == TIER_FULL ? RT_SHADE_BATCH_FULL : RT_SHADE_BATCH_FLAT;
        auto step = [&]() -> bool {
            // every step call of the lane (the basic tier counts its own)
            RT_DIAG_ONLY(if (__lane_id() == (uint32_t)(__ffsll((long long)__ballot(true)) - 1)) ++dg.wave_trace_iters; ++dg.lane_trace_iters;)
            if constexpr (PARK_RAY)
                return trace_step<TIER>(S, RayLds{pst + 9 * RT_BLOCK}, T, stk, rng, med, dg);
            else
                return trace_step<TIER>(S, ray, T, stk, rng, med, dg);
        };
        if constexpr (BATCH >= 64) {  // the whole wave finishes its walks, then shades
            if constexpr (LDS_STATE) {
                pst[0 * RT_BLOCK] = beta.x, pst[1 * RT_BLOCK] = beta.y, pst[2 * RT_BLOCK] = beta.z;
                pst[3 * RT_BLOCK] = L.x, pst[4 * RT_BLOCK] = L.y, pst[5 * RT_BLOCK] = L.z;
                pit[0] = make_uint2(sie, s_j);
                if constexpr (PARK_RAY) {
                    pst[9 * RT_BLOCK] = ray.o.x, pst[10 * RT_BLOCK] = ray.o.y, pst[11 * RT_BLOCK] = ray.o.z;
                    pst[12 * RT_BLOCK] = ray.d.x, pst[13 * RT_BLOCK] = ray.d.y, pst[14 * RT_BLOCK] = ray.d.z;
                    pst[15 * RT_BLOCK] = ray.time;
                }
            }
#ifdef RT_WAVE_TRACE
            while (walking) walking = step(), ++trace_steps;
#else
            while (walking) walking = step();
#endif
            RT_DIAG_ONLY(const unsigned long long t_m0 = __builtin_amdgcn_s_memtime();)
            if constexpr (PARK_RAY)
                media_phase<TIER>(S, RayLds{pst + 9 * RT_BLOCK}, T, stk, rng, med);
            else if constexpr (tier_full(TIER))
                media_phase<TIER>(S, ray, T, stk, rng, med);
            RT_DIAG_ONLY(dg.cyc_media += __builtin_amdgcn_s_memtime() - t_m0;)
            if constexpr (LDS_STATE) {
                if constexpr (PARK_RAY) ray = RayLds{pst + 9 * RT_BLOCK}.get();
                beta = d3(pst[0 * RT_BLOCK], pst[1 * RT_BLOCK], pst[2 * RT_BLOCK]);
                L = d3(pst[3 * RT_BLOCK], pst[4 * RT_BLOCK], pst[5 * RT_BLOCK]);
                const uint2 it = pit[0];
                sie = it.x, s_j = it.y;
            }
        } else {
            const unsigned long long active = __ballot(true);
            for (;;) {
                if (walking) walking = step();
                const unsigned long long w = __ballot(walking);
                if (w == 0 || __popcll(active & ~w) >= BATCH) break;
            }
        }
        RT_DIAG_ONLY(const unsigned long long t_b1 = __builtin_amdgcn_s_memtime(); dg.cyc_trace += t_b1 - t_b0;)
        if constexpr (BATCH < 64 && tier_full(TIER)) {
            RT_DIAG_ONLY(const unsigned long long t_mb = __builtin_amdgcn_s_memtime();)
            if (!walking) media_phase<TIER>(S, ray, T, stk, rng, med);
            RT_DIAG_ONLY(dg.cyc_media += __builtin_amdgcn_s_memtime() - t_mb;)
        }
        if (BATCH < 64 && walking) {
            if constexpr (PARK) trace_park(T, pk);
            continue;
        }
        bool panic = false;
        Draws Dr{};
        if constexpr (!tier_full(TIER)) {  // (the mesh tier: the shading draws made here)
            if (T.found) {
                uint32_t ovf = 0;
                Dr.xi0 = rng.next(ovf);
                Dr.xi1 = rng.next(ovf);
                k_sincos_2pi(Dr.xi0, &Dr.sn, &Dr.cs);
            }
        }
#ifdef RT_DIAG
        {  // the round's shading classes (diagnostic build): one dependent load for the material
            uint32_t cls = 0;  // miss
            if (T.found) {
                const uint32_t k = ref_kind(T.hit.ref), i = ref_index(T.hit.ref);
                const int32_t m = k == K_SPHERE ? S.sphere_mat[i] : k == K_MSPHERE ? S.msph_mat[i]
                                : (k == K_QUAD || k == K_TRI) ? S.planar_mat[i] : k == K_MEDIUM ? S.media[i].phase_mat : -1;
                const int32_t mt = m >= 0 ? S.materials[m].type : -1;
                cls = mt == M_LAMBERTIAN ? 1u + (uint32_t)min(S.textures[S.materials[m].tex].type, 4)
                    : mt == M_METAL ? 6u : mt == M_DIELECTRIC ? 7u : mt == M_DIFFUSE_LIGHT ? 8u : mt == M_ISOTROPIC ? 9u : 10u;
            }
            const unsigned long long act = __ballot(true);
            uint32_t kinds = 0;
            const bool first = __lane_id() == (uint32_t)(__ffsll((long long)act) - 1);
            for (uint32_t c = 0; c <= 10u; ++c) {
                const unsigned long long bc = __ballot(cls == c);
                kinds += bc != 0ull ? 1u : 0u;
                if (first && bc) {
                    ++dg.cls_rounds[c];
                    dg.cls_lanes[c] += (unsigned long long)__popcll(bc);
                }
            }
            if (first) {
                ++dg.sh_rounds;
                dg.sh_lanes += (unsigned long long)__popcll(act);
                dg.sh_classes += kinds;
            }
        }
#endif
        bool end_path = shade<TIER>(S, ray, beta, L, rng, T.found, T.hit, panic, Dr);
        RT_DIAG_ONLY(dg.cyc_shade += __builtin_amdgcn_s_memtime() - t_b1;)
        if (panic) {
            ++n_panics;
            end_path = true;
        }
        if (!end_path) {
            ++vertex;
            if (vertex > F.max_depth) {  // depth == 0 -> BLACK (camera.rs:282-284)
                end_path = true;
                // the recursion multiplies that BLACK by every level's f / pdf on its way up: a non-finite
                // one (Disney's pdf = NaN at a zero weight sum) makes it NaN there (camera.rs:323)
                if constexpr (TIER == TIER_FULL_DS) L = L + beta * d3(0, 0, 0);
            }
        }
        if (end_path) {
            if (isnan(L.x) || isnan(L.y) || isnan(L.z)) {  // camera.rs:323
                ++n_panics;
                L = d3(0, 0, 0);
            }
            in_path = false;
            ++s_j;
            if constexpr (ACC_LDS) {
                const D3 a = d3(pst[6 * RT_BLOCK], pst[7 * RT_BLOCK], pst[8 * RT_BLOCK]) + L;
                if (s_j == (sie >> 16)) {
                    double* dst = P->partial + (uint64_t)pit[BLK].y * 3;
                    dst[0] = a.x;
                    dst[1] = a.y;
                    dst[2] = a.z;
                    need = true;
                } else {
                    pst[6 * RT_BLOCK] = a.x, pst[7 * RT_BLOCK] = a.y, pst[8 * RT_BLOCK] = a.z;
                }
            } else {
                acc = acc + L;
                if (s_j == (sie >> 16)) {
                    double* dst = P->partial + (uint64_t)slot * 3;
                    dst[0] = acc.x;
                    dst[1] = acc.y;
                    dst[2] = acc.z;
                    need = true;
                }
            }
        }
    }
    }  // full tiers
    const uint32_t lane = __lane_id();
#ifdef RT_DIAG
    // wave-uniform cycle counts: lane 0 of each wave; lane counters: every lane
    if (lane == 0) {
        atomicAdd(&g_diag[0], dg.cyc_refill);
        atomicAdd(&g_diag[1], dg.cyc_trace);
        atomicAdd(&g_diag[2], dg.cyc_shade);
        atomicAdd(&g_diag[4], dg.main_iters);
        atomicAdd(&g_diag[13], dg.cyc_media);
        atomicAdd(&g_diag[21], dg.cyc_miss);
        atomicAdd(&g_diag[22], dg.cyc_queue);
        atomicAdd(&g_diag[23], dg.cyc_draws);
    }
    atomicAdd(&g_diag[3], dg.wave_trace_iters);  // counted by the first active lane of each wave iteration
    atomicAdd(&g_diag[5], dg.lane_trace_iters);
    atomicAdd(&g_diag[6], dg.node_visits);
    atomicAdd(&g_diag[7], dg.sphere_tests);
    atomicAdd(&g_diag[8], (unsigned long long)n_rays);
    atomicAdd(&g_diag[9], dg.load_cyc);
    atomicAdd(&g_diag[10], dg.loads);
    atomicAdd(&g_diag[11], dg.pops);
    atomicAdd(&g_diag[12], dg.pop_reads);
    atomicAdd(&g_diag[14], dg.big_tests);
    atomicAdd(&g_diag[15], dg.big_hits);
    atomicAdd(&g_diag[16], dg.u_steps);
    atomicAdd(&g_diag[17], dg.u_uniform);
    atomicAdd(&g_diag[18], dg.u_uniform_node);
    atomicAdd(&g_diag[19], dg.u_active);
    atomicAdd(&g_diag[20], dg.u_same);
    for (int k = 0; k < 4; ++k) {
        atomicAdd(&g_diag[24 + k], dg.u_top[k]);
        atomicAdd(&g_diag[28 + k], dg.l_top[k]);
    }
    atomicAdd(&g_diag[32], dg.l_node);
    // counted by the first active lane of a round, which need not be lane 0
    // (lanes whose walk has ended are masked off): flushed from every lane,
    // as g_diag[3]
    atomicAdd(&g_diag[33], dg.sh_rounds);
    atomicAdd(&g_diag[34], dg.sh_lanes);
    atomicAdd(&g_diag[35], dg.sh_classes);
    atomicAdd(&g_diag[36], dg.pure_rounds);
    atomicAdd(&g_diag[37], dg.pure_lanes);
    atomicAdd(&g_diag[38], dg.pure_max_pn);
    if (lane == 0) atomicAdd(&g_diag[61], dg.cyc_camera);
    atomicAdd(&g_diag[62], dg.prim_rays);
    atomicAdd(&g_diag[63], dg.prim_tests);
    for (int k = 0; k < 11; ++k) {
        atomicAdd(&g_diag[39 + k], dg.cls_rounds[k]);
        atomicAdd(&g_diag[50 + k], dg.cls_lanes[k]);
    }
#endif
#ifdef RT_WAVE_TRACE
    hist.flush();
    if (trace_lane < RT_TRACE_LANES) {
        unsigned long long* t = g_lane_trace + (uint64_t)trace_lane * RT_TRACE_W;
        t[0] = trace_t0;
        t[1] = __builtin_amdgcn_s_memrealtime();
        t[2] = trace_items;
        t[3] = n_rays;
        t[4] = trace_tq;
        t[5] = trace_q;
        t[6] = trace_rays;
        t[7] = __builtin_amdgcn_s_memtime() - trace_c0;  // shader clocks over the lane's life
        t[8] = trace_steps;  // walk steps (wave iterations the lane walked in)
        t[9] = trace_steps_q;  // ... at its last refill
        t[10] = trace_atomic_ticks | ((unsigned long long)trace_atomics << 40);  // wave's atomic wait, count
        t[11] = trace_atomic_first;  // when the wave's first atomic returned (ticks after its start)
    }
#endif
    // one atomic per wave, not per lane: 262 144 adds to one address at the
    // end of every launch
    uint32_t rays_w = n_rays, panics_w = n_panics;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        rays_w += __shfl_xor(rays_w, o);
        panics_w += __shfl_xor(panics_w, o);
    }
    if (lane == 0) {
        atomicAdd(&P->stats[0], (unsigned long long)rays_w);
        if (panics_w) atomicAdd(&P->stats[1], (unsigned long long)panics_w);
    }
}

}  // namespace rtk

#define RT_TIER_ENTRY(N)                                                                                        \
    extern "C" hipError_t rtk_launch_path_##N(int grid, hipStream_t stream, const rtk::KParams* P) {          \
        hipLaunchKernelGGL(rtk::rt_path_kernel<N>, dim3(grid), dim3(N == 0 ? RT_BLOCK_BASIC : RT_BLOCK), 0, stream, P); \
        return hipGetLastError();                                                                            \
    }                                                                                                        \
    extern "C" int rtk_occupancy_##N(int* blocks_per_cu) {                                                   \
        return (int)hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, rtk::rt_path_kernel<N>,            \
                                                                 N == 0 ? RT_BLOCK_BASIC : RT_BLOCK, 0);         \
    }
#if !defined(RT_TIER) || RT_TIER == 0
RT_TIER_ENTRY(0)
// the basic tier's wide variant (trees past NODE_LDS_CAP_BATCH nodes)
extern "C" hipError_t rtk_launch_path_0w(int grid, hipStream_t stream, const rtk::KParams* P) {
    hipLaunchKernelGGL((rtk::rt_path_kernel<0, true>), dim3(grid), dim3(RT_BLOCK_BASIC), 0, stream, P);
    return hipGetLastError();
}
#endif
#if !defined(RT_TIER) || RT_TIER == 1
RT_TIER_ENTRY(1)
#endif
#if !defined(RT_TIER) || RT_TIER == 2
RT_TIER_ENTRY(2)
#endif
#if !defined(RT_TIER) || RT_TIER == 3
RT_TIER_ENTRY(3)
#endif
#if !defined(RT_TIER) || RT_TIER == 4
RT_TIER_ENTRY(4)
#endif
#if !defined(RT_TIER) || RT_TIER == 5
RT_TIER_ENTRY(5)

// Disney self-test (rt_disney_selftest): the device functions shade<TIER_FULL_DS>
// calls, in this tier's object and so under its flags, one case per thread.
//  fn 0  Disney::evaluate_disney: local v_out[3], local v_in[3], front_face
//        -> reflectance[3], forward pdf, reverse pdf, panic
//  fn 1  Disney::scatter's v_out + DisneyPDF::new + generate, the draws given:
//        world normal[3], world -r_in.direction[3], front_face, four unit draws
//        in call order -> 1 / 0 (Some / None), direction[3], draws consumed, panic
// A case that panics writes zeros and the flag.
namespace rtk {
__global__ void __launch_bounds__(256) rt_disney_kernel(int fn, DDisney R, D3 base_color, int in_w, int out_w,
                                                       const double* __restrict__ in, double* __restrict__ out,
                                                       uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* p = in + i * (uint64_t)in_w;
    double* q = out + i * (uint64_t)out_w;
    disney::Params P;
    P.base_color = base_color;
    P.roughness = R.roughness, P.anisotropic = R.anisotropic, P.sheen = R.sheen, P.sheen_tint = R.sheen_tint;
    P.clearcoat = R.clearcoat, P.clearcoat_gloss = R.clearcoat_gloss, P.specular_tint = R.specular_tint;
    P.metallic = R.metallic, P.ior = R.ior, P.flatness = R.flatness, P.spec_trans = R.spec_trans;
    P.diff_trans = R.diff_trans;
    P.thin = R.thin != 0;
    bool panic = false;
    double r[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (fn == 0) {
        D3 f;
        double fwd, rev;
        disney::evaluate_disney(P, d3(p[0], p[1], p[2]), d3(p[3], p[4], p[5]), p[6] != 0.0, f, fwd, rev, panic);
        r[0] = f.x, r[1] = f.y, r[2] = f.z, r[3] = fwd, r[4] = rev;
    } else {
        const disney::Pdf pdf = disney::pdf_new(d3(p[0], p[1], p[2]), d3(p[3], p[4], p[5]), p[6] != 0.0, panic);
        if (!panic) {
            const double u[4] = {p[7], p[8], p[9], p[10]};
            disney::ArrayDraw dr{u, 0};
            D3 dir = d3(0.0, 0.0, 0.0);
            const bool some = disney::generate_impl(P, pdf, dr, dir, panic);
            r[0] = some ? 1.0 : 0.0;
            if (some) r[1] = dir.x, r[2] = dir.y, r[3] = dir.z;
            r[4] = (double)dr.n;
        }
    }
    for (int k = 0; k < 5; ++k) q[k] = panic ? 0.0 : r[k];
    q[5] = panic ? 1.0 : 0.0;
}
}  // namespace rtk

extern "C" int rtk_disney_widths(int fn, int* in_w, int* out_w) {
    if (fn < 0 || fn > 1) return 0;
    *in_w = fn == 0 ? 7 : 11;
    *out_w = 6;
    return 1;
}

extern "C" hipError_t rtk_launch_disney(int fn, const rt_disney_params* params, const double* base_color,
                                        const double* in, double* out, uint64_t n, hipStream_t stream) {
    int in_w = 0, out_w = 0;
    if (!rtk_disney_widths(fn, &in_w, &out_w)) return hipErrorInvalidValue;
    if (n == 0) return hipSuccess;
    rtk::DDisney R{};
    R.roughness = params->roughness, R.anisotropic = params->anisotropic, R.sheen = params->sheen;
    R.sheen_tint = params->sheen_tint, R.clearcoat = params->clearcoat, R.clearcoat_gloss = params->clearcoat_gloss;
    R.specular_tint = params->specular_tint, R.metallic = params->metallic, R.ior = params->ior;
    R.flatness = params->flatness, R.spec_trans = params->spec_trans, R.diff_trans = params->diff_trans;
    R.thin = params->thin != 0;
    hipLaunchKernelGGL(rtk::rt_disney_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, fn, R,
                       rtk::D3{base_color[0], base_color[1], base_color[2]}, in_w, out_w, in, out, n);
    return hipGetLastError();
}
#endif
#if defined(RT_WAVE_TRACE)
extern "C" int rt_lane_trace(unsigned long long* out, uint64_t n_lanes) {
    if (n_lanes > rtk::RT_TRACE_LANES) n_lanes = rtk::RT_TRACE_LANES;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(rtk::g_lane_trace),
                                    n_lanes * rtk::RT_TRACE_W * sizeof(unsigned long long));
}
// the rays-begun histogram (RT_HIST_N buckets of 0.25 ms); out == NULL: zero it
extern "C" int rt_ray_hist(unsigned long long* out, uint64_t n) {
    static const unsigned long long zero[rtk::RT_HIST_N] = {};
    if (!out) return (int)hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_ray_hist), zero, sizeof zero);
    if (n > rtk::RT_HIST_N) n = rtk::RT_HIST_N;
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(rtk::g_ray_hist), n * sizeof(unsigned long long));
}
#endif
#if defined(RT_CHECK)
// check build: {refs past their arrays, 1 << 32 | the first bad ref} on the
// current device (rt_render.cpp wait())
extern "C" int rtk_check_read(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(rtk::g_check), sizeof(unsigned long long) * 2);
    if (reset) {
        unsigned long long z[2] = {};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_check), z, sizeof z);
    }
    return (int)e;
}
#endif
#if defined(RT_DIAG)
// diagnostic build: the counters live with the (DIAG_TIER) kernel that adds to them
extern "C" int rt_diag_counters(unsigned long long* out, int reset) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(rtk::g_diag), sizeof(unsigned long long) * rtk::RT_DIAG_N);
    if (reset) {
        unsigned long long z[rtk::RT_DIAG_N] = {};
        (void)hipMemcpyToSymbol(HIP_SYMBOL(rtk::g_diag), z, sizeof z);
    }
    return (int)e;
}
#endif
