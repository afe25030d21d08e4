// rt_kernel_occl.hip -- rt_world_occluded's kernels (rt_occl_kernel) and their
// host entry point.  An object of its own in the product build, as the hit
// query's is: no other kernel object sees a further caller of the walk.
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_builds.h"
#include "rt_geom.h"
#include "rt_stack.h"
#include "rt_walk.h"
#include "rt_walk4.h"

namespace rtk {

// ------------------------------------------------------------------ occlusion queries
// rt_world_occluded: world.hit(Ray{origin, dir, time}, [1e-8, t_max]).is_some()
// (hit.rs:46-60) for n caller-given rays, one ray per lane and one byte each:
// rt_hit_kernel's walk, ended at the first accepted hit, without make_record.
//
// Why the early end is exact.  The byte is T.found of the closest-hit walk
// when it and its media phase are over, and found never goes back to false:
//  - a solid hit anywhere in the interval makes hit return Some, whatever a
//    closer surface or a medium then does to the record;
//  - a medium tested inside the walk (a full media queue, rt_walk.h
//    trace_step K_MEDIUM) that hits does the same;
//  - up to its first accepted hit this walk is the closest-hit walk step for
//    step -- the same stack, the same closest bound (t_max), the same queued
//    media -- so where the walk finds nothing it ends as that walk does, and
//    media_phase sees the same bound and draws the same medium stream of
//    (seed, pixel = the ray's index, sample 0, vertex 1).
// So media_phase runs only where the finished walk found nothing, and a walk
// that found something is dropped where it stands: words left on its stack,
// spheres left in its queue and media left in its queue belong to no one, and
// the lane's next ray begins from trace_begin's empty state.
struct OcclParams {
    SceneView S;
    const rt_ray* rays;
    uint8_t* out;
    uint64_t n;  // < 2^32 (the host's check): a ray's index is its Rng pixel
    uint32_t key0, key1;
    RT_GLOBAL uint2* stack_ovf;  // mesh / full tiers: [stack_need - LDS entries][grid * RT_BLOCK]
};

template <int TIER>
__global__ void __launch_bounds__(TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK) rt_occl_kernel(const OcclParams P) {
    const SceneView& S = P.S;
    constexpr int STACK = lds_stack_entries(TIER);
    constexpr uint32_t BLK = TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    constexpr bool B4 = TIER == TIER_BASIC;
    // rt_hit_kernel's LDS set-up
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
    Diag dg;
    Rng rng;
    rng.k0 = P.key0;
    rng.k1 = P.key1;
    rng.sample = 0;
    // Grid-stride over the rays, a wave at a time, as rt_hit_kernel: the 64
    // lanes of a wave make the same trips and the lanes past n come along
    // with no ray (the last wave only).  (A second form, in which a lane
    // whose ray is done takes the wave's next ray between steps, was built and
    // measured against this one and not kept: DESIGN.md §9, round 16.)
    const uint64_t stride = (uint64_t)gridDim.x * BLK;
    for (uint64_t w0 = (uint64_t)blockIdx.x * BLK + (threadIdx.x & ~63u); w0 < P.n; w0 += stride) {
        const uint64_t i = w0 + (threadIdx.x & 63u);
        const bool live = i < P.n;
        Ray ray{};
        double t_max = 0.0;
        if (live) {
            const rt_ray q = P.rays[i];
            ray.o = d3(q.origin[0], q.origin[1], q.origin[2]);
            ray.d = d3(q.dir[0], q.dir[1], q.dir[2]);
            ray.time = q.time;
            t_max = q.t_max;
        }
        rng.pixel = (uint32_t)i;
        rng.begin(1);
        Trav<TIER> T;
        trace_begin<TIER>(S, ray, T);
        T.cl.set(t_max);
        if constexpr (B4) {
            // trace4_step ballots across the wave, so every lane takes every
            // step in wave-uniform control flow (rt_hit_kernel).  A lane that
            // has found a hit takes the empty walk state: the next step does
            // nothing for it and returns false, and since the step counts its
            // sphere-round threshold from the state's own masks, the lanes
            // that dropped out lower it without further code.
            if (!live) T.cur = 0u;
            bool walking = live;
            while (__ballot(walking)) {
                walking = trace4_step(S, ray, T, stk, pq, (const RT_LDS float4*)node_lds, dg);
                if (T.found) {
                    T.cur = 0u;
                    T.sp = 0;
                    T.pn = 0;
                    walking = false;
                }
            }
        } else if (live) {
            // (trace_step holds no cross-lane operation: each lane walks on its own)
            while (!T.found && trace_step<TIER>(S, ray, T, stk, rng, med, dg)) {
            }
            if constexpr (tier_full(TIER)) {
                if (!T.found) media_phase<TIER>(S, ray, T, stk, rng, med);
            }
        }
        if (live) P.out[i] = T.found ? (uint8_t)1 : (uint8_t)0;
    }
}

}  // namespace rtk

// n rays through world.hit(..).is_some() (rt_world_occluded): rays and out are
// device arrays; grid blocks of the tier's block size, at most the path
// kernel's grid -- stack_ovf is sized for that many lanes (rt_render.cpp
// upload_world).
extern "C" hipError_t rtk_launch_occluded(const rtk::SceneView* view, const rt_ray* rays, uint8_t* out, uint64_t n,
                                          uint64_t seed, int tier, int grid, void* stack_ovf, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    rtk::OcclParams P;
    P.S = *view;
    P.rays = rays;
    P.out = out;
    P.n = n;
    P.key0 = (uint32_t)seed;
    P.key1 = (uint32_t)(seed >> 32);
    P.stack_ovf = (RT_GLOBAL uint2*)stack_ovf;
    const int block = tier == rtk::TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    const uint64_t blocks = (n + (uint64_t)block - 1) / (uint64_t)block;
    const dim3 g((unsigned)(blocks < (uint64_t)grid ? blocks : (uint64_t)grid)), b((unsigned)block);
    switch (tier) {
        case rtk::TIER_BASIC: hipLaunchKernelGGL(rtk::rt_occl_kernel<rtk::TIER_BASIC>, g, b, 0, stream, P); break;
        case rtk::TIER_MESH: hipLaunchKernelGGL(rtk::rt_occl_kernel<rtk::TIER_MESH>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL: hipLaunchKernelGGL(rtk::rt_occl_kernel<rtk::TIER_FULL>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL_FLAT: hipLaunchKernelGGL(rtk::rt_occl_kernel<rtk::TIER_FULL_FLAT>, g, b, 0, stream, P); break;
        default: return hipErrorInvalidValue;  // (lights = -1: no world selects TIER_FULL_GL)
    }
    return hipGetLastError();
}
