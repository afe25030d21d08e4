// rt_kernel_hit.hip -- rt_world_hit's kernels (rt_hit_kernel) and their host
// entry point.  An object of its own in the product build, so that no
// path-kernel object sees a second caller of the walk or of make_record.
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_builds.h"
#include "rt_geom.h"
#include "rt_stack.h"
#include "rt_walk.h"
#include "rt_walk4.h"
#include "rt_record.h"

namespace rtk {

// ------------------------------------------------------------------ hit queries
// rt_world_hit: world.hit(Ray{origin, dir, time}, [1e-8, t_max]) (hit.rs:46-60)
// for n caller-given rays, one ray per lane, and the HitRecord each returns
// (hit.rs:24-43) -- the path kernels' walk and record, called as they call
// them: trace_begin, trace4_step (basic tier) or trace_step and media_phase,
// then make_record in its query mode.  t_max enters as the walk's initial
// closest bound with nothing found, so a hit at exactly t_max is accepted
// (interval.rs:65-67) and one past it is not.  A ConstantMedium's draw is the
// contract's medium stream of (seed, pixel = the ray's index, sample 0,
// vertex 1).
struct HitParams {
    SceneView S;
    const rt_ray* rays;
    rt_hit_record* out;
    uint64_t n;  // < 2^32 (the host's check): a ray's index is its Rng pixel
    uint32_t key0, key1;
    RT_GLOBAL uint2* stack_ovf;  // mesh / full tiers: [stack_need - LDS entries][grid * RT_BLOCK]
};

template <int TIER>
__global__ void __launch_bounds__(TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK) rt_hit_kernel(const HitParams P) {
    const SceneView& S = P.S;
    constexpr int STACK = lds_stack_entries(TIER);
    constexpr uint32_t BLK = TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    constexpr bool B4 = TIER == TIER_BASIC;
    // the path kernel's LDS set-up without its parked path state: the lane
    // arena (stack rows, then the full tiers' media queue), or the basic
    // tier's 4-B stack, sphere queue and whole node copy (as its WIDE variant)
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
    // Grid-stride over the rays, a wave at a time: the loop's bound is the
    // wave's first ray, so the 64 lanes of a wave make the same trips and the
    // lanes past n come along with no ray (the last wave only).
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
            // A lane with no ray holds the empty walk state (no word to walk,
            // nothing queued: rt_path_kernel).  trace4_step ballots across
            // the wave, so it is called in wave-uniform control flow, as the
            // path kernel's batch loop calls it: every lane of the wave takes
            // every step until none walks any more, and a step on a finished
            // or empty walk does nothing and returns false.
            if (!live) T.cur = 0u;
            bool walking = live;
            while (__ballot(walking))
                walking = trace4_step(S, ray, T, stk, pq, (const RT_LDS float4*)node_lds, dg);
        } else if (live) {
            // (trace_step holds no cross-lane operation: each lane walks on its own)
            while (trace_step<TIER>(S, ray, T, stk, rng, med, dg)) {
            }
            if constexpr (tier_full(TIER)) media_phase<TIER>(S, ray, T, stk, rng, med);
        }
        if (live) {
            rt_hit_record o{};  // a miss: flags 0, mat -1, every double 0
            o.mat = -1;
            if (T.found) {
                bool panic = false;  // (remap_record's unwraps: not reached in query mode)
                const Rec rec = make_record<TIER, true>(S, ray, T.hit, panic);
                o.t = T.hit.t;
                o.p[0] = rec.p.x, o.p[1] = rec.p.y, o.p[2] = rec.p.z;
                o.normal[0] = rec.n.x, o.normal[1] = rec.n.y, o.normal[2] = rec.n.z;
                o.u = rec.u;
                o.v = rec.v;
                o.mat = rec.mat;
                o.flags = RT_HIT_FOUND | (rec.front ? RT_HIT_FRONT_FACE : 0u) |
                          (ref_kind(T.hit.ref) == K_MEDIUM ? RT_HIT_MEDIUM : 0u);
            }
            P.out[i] = o;
        }
    }
}

}  // namespace rtk

// n rays through world.hit (rt_world_hit): rays and out are device arrays;
// grid blocks of the tier's block size, at most the path kernel's grid --
// stack_ovf is sized for that many lanes (rt_render.cpp upload_world).
extern "C" hipError_t rtk_launch_hits(const rtk::SceneView* view, const rt_ray* rays, rt_hit_record* out, uint64_t n,
                                      uint64_t seed, int tier, int grid, void* stack_ovf, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    rtk::HitParams P;
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
        case rtk::TIER_BASIC: hipLaunchKernelGGL(rtk::rt_hit_kernel<rtk::TIER_BASIC>, g, b, 0, stream, P); break;
        case rtk::TIER_MESH: hipLaunchKernelGGL(rtk::rt_hit_kernel<rtk::TIER_MESH>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL: hipLaunchKernelGGL(rtk::rt_hit_kernel<rtk::TIER_FULL>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL_FLAT: hipLaunchKernelGGL(rtk::rt_hit_kernel<rtk::TIER_FULL_FLAT>, g, b, 0, stream, P); break;
        default: return hipErrorInvalidValue;  // (lights = -1: no world selects TIER_FULL_GL)
    }
    return hipGetLastError();
}
