// rt_kernel_radiance.hip -- rt_world_radiance's kernels (rt_radiance_kernel of
// the six tiers) and their host entry point.  An object of its own in the
// product build, as the hit and occlusion queries' are: no path-kernel object
// sees a second caller of the walk or of shade.
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_queue.h"
#include "rt_builds.h"
#include "rt_texture.h"
#include "rt_geom.h"
#include "rt_stack.h"
#include "rt_walk.h"
#include "rt_walk4.h"
#include "rt_record.h"
#include "rt_lights.h"
#include "rt_shade.h"

namespace rtk {

// ------------------------------------------------------------------ radiance queries
// rt_world_radiance: Camera::ray_color(Ray{origin, dir, time}, max_depth, world,
// lights) (camera.rs:275-325) for n caller-given rays, `samples` times each --
// the path kernel's round without its camera: rng.begin(vertex), trace_begin,
// the walk to its end (trace4_step on the basic tier, trace_step and
// media_phase elsewhere), the vertex's draws where the tier hoists them, shade
// (shade_hit_basic for the basic tier's hits), and the panic / depth / NaN
// handling in the path kernel's order.  The caller's t_max enters as the first
// walk's initial closest bound with nothing found, as in rt_hit_kernel: a first
// hit past it is a miss and the background is returned; every later vertex
// walks [1e-8, inf).
//
// Work items are rays.  A lane does the samples of its ray in ascending order
// and sums them in f64 from zero, then scales once by 1 / samples, so the sum
// does not depend on which lane ran the ray; the Rng of sample s of ray i is
// (key, pixel = first_index + i, sample = s, vertex = 1, 2, ...), what
// rt_render draws from vertex 1 on.
//
// Refill.  A lane's first ray is its own index in the grid: no atomic at
// launch.  A lane whose ray is done takes the next one from its wave's pool
// of ray indices [next, end), in the rank order of the wave's lanes in need
// (__ballot, popcount, mbcnt); a pool that runs short is filled by one
// atomicAdd on a device-wide counter, made by the first lane in need, which
// hands out the rays from the grid's lane count on.  The chunk a wave takes
// is rt_queue.h's guided one in its simplest form -- the rays left, as last
// seen, over the grid's waves times RT_QUEUE_GUIDE, at most RT_QUEUE_CHUNK and
// at least what the lanes need now -- so pools shrink to nothing as the batch
// runs out and no wave sits on rays another could run.  (One atomic per
// refill with no pool was measured first: about a million adds to one address
// on C2, 12.2 ms a query against 9.2 with the pool, and 15.8 against 6.7 at
// one sample a ray; DESIGN.md.)  Lanes therefore stay
// busy until the counter passes n, whatever the lengths of their neighbours'
// paths.  The pool is wave-uniform state in scalar registers, updated where
// the wave's remaining lanes are together: at the head of the loop.
struct RadParams {
    SceneView S;
    const rt_ray* rays;
    rt_radiance* out;
    uint32_t n;            // rays of this launch, <= 2^31 (rtk_launch_radiance)
    uint32_t first_index;  // the Rng pixel of ray 0
    uint32_t samples, max_depth;  // both >= 1 (max_depth 0 never launches)
    uint32_t key0, key1;
    uint32_t* counter;           // zero at launch: the rays handed out past the grid's lane count
    RT_GLOBAL uint2* stack_ovf;  // mesh / full tiers: [stack_need - LDS entries][grid * RT_BLOCK]
};

// waves per SIMD the tier's path kernel is register-allocated for
// (rt_kernel_path.hip RT_BASIC_WAVES, RT_MESH_WAVES, RT_FULL_WAVES,
// RT_FLAT_WAVES): the same budget here, so that the path kernel's grid, for
// which stack_ovf is sized, is resident at once
constexpr int radiance_waves(int tier) {
    return tier == TIER_FULL_FLAT ? 3 : tier_full_bvh(tier) ? 2 : 4;
}

template <int TIER>
__global__ void __launch_bounds__(TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK, radiance_waves(TIER))
    rt_radiance_kernel(const RadParams P) {
    const SceneView& S = P.S;
    constexpr int STACK = lds_stack_entries(TIER);
    constexpr uint32_t BLK = TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    constexpr bool B4 = TIER == TIER_BASIC;
    // rt_hit_kernel's LDS set-up: the lane arena (stack rows, then the full
    // tiers' media queue), or the basic tier's 4-B stack, sphere queue and
    // whole node copy (its wide variant) ...
    constexpr uint32_t R_MED = lane_rows_med<TIER>();
    constexpr uint32_t R_END = R_MED + (tier_full(TIER) ? 2u * RT_MEDIA_CAP : 0u);
    __shared__ uint2 lane_lds[B4 ? 1 : R_END * BLK];
    __shared__ uint32_t stack4_lds[B4 ? STACK * BLK : 1];
    __shared__ uint16_t pend_lds[B4 ? RT_PEND_CAP * BLK : 1];
    __shared__ float4 node_lds[B4 ? NODE_LDS_CAP * 7 : 1];
    const WalkLds<TIER> wl = walk_lds<TIER>(lane_lds, stack4_lds, pend_lds, P.stack_ovf);
    const MedQ med = wl.med;
    RT_LDS uint16_t* pq = wl.pq;
    StackFor<TIER> stk = wl.stk;
    if constexpr (B4) RT_COPY_NODES_LDS(S, node_lds, NODE_LDS_CAP, BLK);
    // ... and what shade reads from the block: the BVH full tiers' copy of the
    // first Perlin table (rt_shade.h PL), as the path kernel makes it
    if constexpr (tier_full_bvh(TIER)) {
        if (S.n_perlin > 0) {
            const RT_GLOBAL float4* src = reinterpret_cast<const RT_GLOBAL float4*>(S.perlin);
            RT_LDS float4* dst = (RT_LDS float4*)&g_perlin_lds;
            for (uint32_t k = threadIdx.x; k < sizeof(DPerlin) / 16; k += BLK) dst[k] = src[k];
            __syncthreads();
        }
    }
    Diag dg;
    Rng rng;
    rng.k0 = P.key0;
    rng.k1 = P.key1;
    rng.pixel = 0;
    rng.sample = 0;
    // the lane's ray (index `item`, sample s of P.samples) and its path; the
    // first ray is the lane's own index
    uint32_t item = blockIdx.x * BLK + threadIdx.x, s = 0;
    bool need = false;        // the lane takes a ray at the next refill
    bool done = item >= P.n;  // no ray for this lane any more
    bool in_path = false;     // a sample of the ray is under way
    rng.pixel = P.first_index + item;
    // the wave's pool of ray indices, and whether an atomic of this wave has
    // passed n (none will hand out a ray any more): wave-uniform
    const uint32_t grid_lanes = gridDim.x * BLK, grid_waves = gridDim.x * (BLK / 64);
    uint32_t pool_next = 0, pool_end = 0;
    bool dry = grid_lanes >= P.n;
    Ray ray{};             // (defined from the start: the basic tier sets up a walk for idle lanes too)
    D3 beta = d3(1, 1, 1), L = d3(0, 0, 0);
    uint32_t vertex = 1;
    // The ray's running sum and counts live in its record, out[item], between
    // its samples -- read, added to and written back at each sample's end by
    // the one lane that owns the ray -- not in ten registers held across the
    // walk and shade: the general tiers spill less for it.
    for (;;) {
        // ---- refill: the lanes in need take rays from the wave's pool, which
        // one atomic fills when it runs short.  The basic tier's lanes are
        // all here (its loop is wave-uniform); elsewhere the ballot is over
        // the lanes that have not left, which is all the rank and the
        // leader are taken from.
        {
            const unsigned long long mask = __ballot(need);
            if (mask) {
                const uint32_t cnt = (uint32_t)__popcll(mask);
                const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                                __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                const uint32_t old_next = pool_next, avail = pool_end - pool_next;
                uint32_t fresh = P.n;  // (the index no lane runs)
                if (avail < cnt) {
                    const uint32_t short_by = cnt - avail;
                    if (!dry) {
                        // (the counter has handed out at least up to the pool's end, and the grid's lanes before it)
                        const uint32_t seen = q_max(pool_end, grid_lanes);
                        const uint32_t left = seen < P.n ? P.n - seen : 0u;
                        const uint32_t chunk = q_uniform(
                            q_max(q_min(left / (grid_waves * (uint32_t)RT_QUEUE_GUIDE), (uint32_t)RT_QUEUE_CHUNK), short_by));
                        const uint32_t leader = __ffsll((long long)mask) - 1;
                        uint32_t got = 0;
                        if (need && rank == 0) got = atomicAdd(P.counter, chunk);
                        // (n <= 2^31 and every wave stops asking once dry: no sum here wraps)
                        fresh = q_uniform(__builtin_amdgcn_readlane(got, leader) + grid_lanes);
                        dry = q_uniform(fresh + chunk >= P.n ? 1u : 0u) != 0u;
                        pool_next = q_uniform(fresh + short_by);
                        pool_end = q_uniform(fresh + chunk);
                    } else {
                        pool_next = pool_end;
                    }
                } else {
                    pool_next = q_uniform(old_next + cnt);
                }
                if (need) {
                    need = false;
                    const uint32_t q = rank < avail ? old_next + rank : (fresh < P.n ? fresh + (rank - avail) : P.n);
                    if (q >= P.n) {
                        done = true;
                    } else {
                        item = q;
                        s = 0;
                        rng.pixel = P.first_index + item;
                    }
                }
            }
        }
        if constexpr (B4) {
            if (!__ballot(!done)) break;
        } else {
            if (done) break;
        }
        // ---- a new sample of the lane's ray: the caller's ray as given
        double t_max = 0.0;
        const bool first_walk = !done && !in_path;
        if (first_walk) {
            const rt_ray q = P.rays[item];
            ray.o = d3(q.origin[0], q.origin[1], q.origin[2]);
            ray.d = d3(q.dir[0], q.dir[1], q.dir[2]);
            ray.time = q.time;
            t_max = q.t_max;
            rng.sample = s;
            beta = d3(1, 1, 1);
            L = d3(0, 0, 0);
            vertex = 1;
            in_path = true;
        }
        // ---- one ray_color level (camera.rs:275-325) at depth max_depth - vertex + 1
        Trav<TIER> T;
        trace_begin<TIER>(S, ray, T);
        if (in_path) {
            rng.begin(vertex);
            if (first_walk) T.cl.set(t_max);  // bounds the first world.hit only
        }
        if constexpr (B4) {
            // trace4_step ballots across the wave, so every lane takes every
            // step in wave-uniform control flow (rt_hit_kernel): a lane with
            // no ray left holds the empty walk state, on which a step does
            // nothing and returns false
            if (!in_path) T.cur = 0u;
            bool walking = in_path;
            while (__ballot(walking))
                walking = trace4_step(S, ray, T, stk, pq, (const RT_LDS float4*)node_lds, dg);
        } else {
            // (trace_step holds no cross-lane operation: each lane walks on its own)
            while (trace_step<TIER>(S, ray, T, stk, rng, med, dg)) {
            }
            if constexpr (tier_full(TIER)) media_phase<TIER>(S, ray, T, stk, rng, med);
        }
        if (!in_path) continue;  // (a basic-tier lane without a ray: back to the loop's head with its wave)
        bool panic = false;
        bool end_path;
        if constexpr (B4) {
            if (T.found) {
                // the vertex's draws (slots 0 and 1) and the merged hit stages
                Draws Dr;
                rng.pair(vertex, 0u, Dr.xi0, Dr.xi1);
                k_sincos_2pi(Dr.xi0, &Dr.sn, &Dr.cs);
                rng.slot = 2;  // slots 0 and 1 are Dr
                end_path = shade_hit_basic(S, ray, beta, T.hit, panic, Dr);
            } else {  // a miss: Environment::value, and the sample ends
                end_path = shade<TIER>(S, ray, beta, L, rng, false, T.hit, panic);
            }
        } else {
            Draws Dr{};
            if constexpr (!tier_full(TIER)) {  // (the mesh tier: the shading draws made here)
                if (T.found) {
                    uint32_t ovf = 0;
                    Dr.xi0 = rng.next(ovf);
                    Dr.xi1 = rng.next(ovf);
                    k_sincos_2pi(Dr.xi0, &Dr.sn, &Dr.cs);
                }
            }
            end_path = shade<TIER>(S, ray, beta, L, rng, T.found, T.hit, panic, Dr);
        }
        if (panic) end_path = true;
        if (!end_path) {
            ++vertex;
            if (vertex > P.max_depth) {  // depth == 0 -> BLACK (camera.rs:282-284)
                end_path = true;
                // as the path kernel: BLACK times a non-finite f / pdf on the recursion's way up is NaN
                if constexpr (TIER == TIER_FULL_DS) L = L + beta * d3(0, 0, 0);
            }
        }
        if (end_path) {
            // the sample's end: a panicked sample adds the radiance gathered
            // so far, or black if that is NaN (camera.rs:323), and counts once
            if (isnan(L.x) || isnan(L.y) || isnan(L.z)) {
                panic = true;
                L = d3(0, 0, 0);
            }
            rt_radiance o{};  // the sum starts from zero
            if (s > 0) o = P.out[item];
            o.rgb[0] += L.x;
            o.rgb[1] += L.y;
            o.rgb[2] += L.z;
            // the sample's ray_color calls that reached world.hit: one per
            // vertex begun (a path the depth ended began max_depth of them)
            o.rays += vertex < P.max_depth ? vertex : P.max_depth;
            if (panic) ++o.panics;
            in_path = false;
            ++s;
            if (s == P.samples) {
                const double scale = 1.0 / (double)P.samples;
                o.rgb[0] *= scale;
                o.rgb[1] *= scale;
                o.rgb[2] *= scale;
                need = true;
            }
            P.out[item] = o;  // item < n: nothing past out[n - 1]
        }
    }
}

}  // namespace rtk

// ray_color of n rays (rt_world_radiance): rays and out are device arrays;
// `counter` one device word of the scene's work buffers, zeroed here on the
// stream ahead of the kernel; grid blocks of the tier's block size, at most the
// path kernel's grid -- stack_ovf is sized for that many lanes (rt_render.cpp
// upload_world).  n <= 2^32 - first_index, samples >= 1, max_depth >= 1.
extern "C" hipError_t rtk_launch_radiance(const rtk::SceneView* view, const rt_ray* rays, rt_radiance* out, uint64_t n,
                                          uint64_t seed, uint32_t first_index, uint32_t samples, uint32_t max_depth,
                                          uint32_t* counter, int tier, int grid, void* stack_ovf, hipStream_t stream) {
    if (n > (1ull << 32) - first_index || samples == 0 || max_depth == 0 || !counter) return hipErrorInvalidValue;
    rtk::RadParams P;
    P.S = *view;
    P.samples = samples;
    P.max_depth = max_depth;
    P.key0 = (uint32_t)seed;
    P.key1 = (uint32_t)(seed >> 32);
    P.counter = counter;
    P.stack_ovf = (RT_GLOBAL uint2*)stack_ovf;
    const int block = tier == rtk::TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    // At most 2^31 rays a launch: the counter goes past n by up to one request
    // of every lane of the grid, and stays a 32-bit word.
    for (uint64_t at = 0; at < n; at += 1ull << 31) {
        const uint64_t m = n - at < (1ull << 31) ? n - at : (1ull << 31);
        hipError_t e = hipMemsetAsync(counter, 0, sizeof(uint32_t), stream);
        if (e != hipSuccess) return e;
        P.rays = rays + at;
        P.out = out + at;
        P.n = (uint32_t)m;
        P.first_index = first_index + (uint32_t)at;
        const uint64_t blocks = (m + (uint64_t)block - 1) / (uint64_t)block;
        const dim3 g((unsigned)(blocks < (uint64_t)grid ? blocks : (uint64_t)grid)), b((unsigned)block);
        switch (tier) {
            case rtk::TIER_BASIC: hipLaunchKernelGGL(rtk::rt_radiance_kernel<rtk::TIER_BASIC>, g, b, 0, stream, P); break;
            case rtk::TIER_MESH: hipLaunchKernelGGL(rtk::rt_radiance_kernel<rtk::TIER_MESH>, g, b, 0, stream, P); break;
            case rtk::TIER_FULL: hipLaunchKernelGGL(rtk::rt_radiance_kernel<rtk::TIER_FULL>, g, b, 0, stream, P); break;
            case rtk::TIER_FULL_FLAT: hipLaunchKernelGGL(rtk::rt_radiance_kernel<rtk::TIER_FULL_FLAT>, g, b, 0, stream, P); break;
            case rtk::TIER_FULL_GL: hipLaunchKernelGGL(rtk::rt_radiance_kernel<rtk::TIER_FULL_GL>, g, b, 0, stream, P); break;
            case rtk::TIER_FULL_DS: hipLaunchKernelGGL(rtk::rt_radiance_kernel<rtk::TIER_FULL_DS>, g, b, 0, stream, P); break;
            default: return hipErrorInvalidValue;
        }
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}
