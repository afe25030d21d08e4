// rt_kernel_scatter.hip -- rt_world_scatter's kernels (rt_scatter_kernel of the
// six tiers) and their host entry point.  An object of its own in the product
// build, as the other queries' are: the walk, make_record and the materials'
// leaf functions get this caller here, not in a path-kernel object.
#include <hip/hip_runtime.h>

#include "../../include/rt_mi355x.h"
#include "rt_kernel.h"
#include "rt_math.h"
#include "rt_builds.h"
#include "rt_texture.h"
#include "rt_geom.h"
#include "rt_stack.h"
#include "rt_walk.h"
#include "rt_walk4.h"
#include "rt_record.h"
#include "rt_lights.h"
#include "rt_shade.h"
#include "rt_scatter.h"

namespace rtk {

// ------------------------------------------------------------------ scatter queries
// rt_world_scatter: one ray_color level (camera.rs:286-316) for n caller-given
// rays without the recursion and without the lights mix -- rng.begin(vertex),
// the walk as rt_hit_kernel runs it (trace4_step under wave-uniform control
// flow on the basic tier, trace_step and media_phase elsewhere; t_max the
// initial closest bound), make_record in its query mode for the `hit` field
// (rt_world_hit's record), then scatter_level (rt_scatter.h) on the shading
// record.  One ray per lane, grid-stride a wave at a time: a single level is
// short and even, so there are no refill pools and no counter.
//
// The Rng of ray i is (key, pixel = indices ? indices[i] : first_index + i,
// sample, vertex): a result depends on that key and the ray alone.
//
// A lane writes the record's first 80 B (the hit) as soon as it has them and
// the other 144 B after the material code, so that the hit's ten doubles are
// not held across it.
struct ScatterParams {
    SceneView S;
    const rt_ray* rays;
    const double* eval_dirs;  // n x 3 or NULL
    const uint32_t* indices;  // n or NULL
    rt_scatter* out;          // 16-B aligned
    uint64_t n;               // < 2^32 (the host's check)
    uint32_t first_index, sample, vertex;
    uint32_t key0, key1;
    RT_GLOBAL uint2* stack_ovf;  // mesh / full tiers: [stack_need - LDS entries][grid * RT_BLOCK]
};

// waves per SIMD: rt_kernel_radiance.hip's radiance_waves(), the budget of the
// tier's path kernel, for whose grid stack_ovf is sized
constexpr int scatter_waves(int tier) {
    return tier == TIER_FULL_FLAT ? 3 : tier_full_bvh(tier) ? 2 : 4;
}

static_assert(sizeof(rt_scatter) == 224 && sizeof(rt_hit_record) == 80, "rt_scatter is 14 x 16 B, its hit 5 x 16 B");

// N 16-B pieces of a record from registers to global memory.  A lane writes
// its own 224-B record, so store k of a wave touches 64 records at a stride of
// 224 B: 14 instructions over the same 112 lines (the access shape
// rt_kernel_lights.hip's header describes).  Written as 8-B stores the
// compiler merges them to these same 16-B ones
template <int N>
__device__ __forceinline__ void store_pieces(void* dst, const double (&v)[2 * N]) {
    double2* p = (double2*)dst;
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = make_double2(v[2 * k], v[2 * k + 1]);
}

template <int TIER>
__global__ void __launch_bounds__(TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK, scatter_waves(TIER))
    rt_scatter_kernel(const ScatterParams P) {
    const SceneView& S = P.S;
    constexpr int STACK = lds_stack_entries(TIER);
    constexpr uint32_t BLK = TIER == TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    constexpr bool B4 = TIER == TIER_BASIC;
    // rt_radiance_kernel's LDS set-up: the lane arena (stack rows, then the
    // full tiers' media queue), or the basic tier's 4-B stack, sphere queue
    // and whole node copy ...
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
    // ... and the BVH full tiers' copy of the first Perlin table (rt_shade.h PL)
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
    rng.sample = P.sample;
    // rt_hit_kernel's loop: the bound is the wave's first ray, so the 64 lanes
    // of a wave make the same trips and the lanes past n come along with no ray
    const uint64_t stride = (uint64_t)gridDim.x * BLK;
    for (uint64_t w0 = (uint64_t)blockIdx.x * BLK + (threadIdx.x & ~63u); w0 < P.n; w0 += stride) {
        const uint64_t i = w0 + (threadIdx.x & 63u);
        const bool live = i < P.n;
        Ray ray{};
        double t_max = 0.0;
        rng.pixel = P.first_index + (uint32_t)i;
        if (live) {
            const rt_ray q = P.rays[i];
            ray.o = d3(q.origin[0], q.origin[1], q.origin[2]);
            ray.d = d3(q.dir[0], q.dir[1], q.dir[2]);
            ray.time = q.time;
            t_max = q.t_max;
            if (P.indices) rng.pixel = P.indices[i];
        }
        rng.begin(P.vertex);
        Trav<TIER> T;
        trace_begin<TIER>(S, ray, T);
        T.cl.set(t_max);
        if constexpr (B4) {
            // (every lane of the wave takes every step: rt_hit_kernel)
            if (!live) T.cur = 0u;
            bool walking = live;
            while (__ballot(walking))
                walking = trace4_step(S, ray, T, stk, pq, (const RT_LDS float4*)node_lds, dg);
        } else if (live) {
            while (trace_step<TIER>(S, ray, T, stk, rng, med, dg)) {
            }
            if constexpr (tier_full(TIER)) media_phase<TIER>(S, ray, T, stk, rng, med);
        }
        if (!live) continue;
        char* const rec_out = (char*)&P.out[i];  // i < n: nothing past out[n - 1]
        {
            // the hit: rt_hit_kernel's record, a miss flags 0, mat -1, every double 0
            double v[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            int32_t mat = -1;
            uint32_t flags = 0;
            if (T.found) {
                bool qpanic = false;  // (remap_record's unwraps: not reached in query mode)
                const Rec rec = make_record<TIER, true>(S, ray, T.hit, qpanic);
                v[0] = T.hit.t;
                v[1] = rec.p.x, v[2] = rec.p.y, v[3] = rec.p.z;
                v[4] = rec.n.x, v[5] = rec.n.y, v[6] = rec.n.z;
                v[7] = rec.u;
                v[8] = rec.v;
                mat = rec.mat;
                flags = RT_HIT_FOUND | (rec.front ? RT_HIT_FRONT_FACE : 0u) |
                        (ref_kind(T.hit.ref) == K_MEDIUM ? RT_HIT_MEDIUM : 0u);
            }
            v[9] = __hiloint2double((int)flags, mat);  // {mat, flags}: mat the low word
            store_pieces<5>(rec_out, v);
        }
        ScatterOut o{};
        D3 ed = d3(0, 0, 0);
        const bool has_eval = P.eval_dirs != nullptr;
        if (has_eval) ed = d3(P.eval_dirs[3 * i], P.eval_dirs[3 * i + 1], P.eval_dirs[3 * i + 2]);
        scatter_level<TIER>(S, ray, T.found, T.hit, rng, has_eval, ed, o);
        uint32_t draws = rng.slot;  // (a miss has drawn nothing on the main stream: 0)
        if (o.flags & SC_PANIC) {   // flags == RT_SCATTER_PANIC alone, hit stays, every other field 0
            o = ScatterOut{};
            o.flags = SC_PANIC;
            draws = 0;
        }
        const double v[18] = {o.emitted.x, o.emitted.y, o.emitted.z, o.f.x,      o.f.y,      o.f.z,
                              o.pdf,       o.origin.x,  o.origin.y,  o.origin.z, o.dir.x,    o.dir.y,
                              o.dir.z,     o.eval_f.x,  o.eval_f.y,  o.eval_f.z, o.eval_pdf,
                              __hiloint2double((int)draws, (int)o.flags)};  // {flags, draws}: flags the low word
        store_pieces<9>(rec_out + sizeof(rt_hit_record), v);
    }
}

}  // namespace rtk

// One ray_color level of n rays (rt_world_scatter): rays, eval_dirs3 (or NULL),
// indices (or NULL) and out are device arrays, out 16-B aligned; grid blocks of
// the tier's block size, at most the path kernel's grid -- stack_ovf is sized
// for that many lanes (rt_render.cpp upload_world).  n < 2^32.
extern "C" hipError_t rtk_launch_scatter(const rtk::SceneView* view, const rt_ray* rays, const double* eval_dirs3,
                                         const uint32_t* indices, rt_scatter* out, uint64_t n, uint64_t seed,
                                         uint32_t first_index, uint32_t sample, uint32_t vertex, int tier, int grid,
                                         void* stack_ovf, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (n >= (1ull << 32) || ((uintptr_t)out & 15u)) return hipErrorInvalidValue;
    rtk::ScatterParams P;
    P.S = *view;
    P.rays = rays;
    P.eval_dirs = eval_dirs3;
    P.indices = indices;
    P.out = out;
    P.n = n;
    P.first_index = first_index;
    P.sample = sample;
    P.vertex = vertex;
    P.key0 = (uint32_t)seed;
    P.key1 = (uint32_t)(seed >> 32);
    P.stack_ovf = (RT_GLOBAL uint2*)stack_ovf;
    const int block = tier == rtk::TIER_BASIC ? RT_BLOCK_BASIC : RT_BLOCK;
    const uint64_t blocks = (n + (uint64_t)block - 1) / (uint64_t)block;
    const dim3 g((unsigned)(blocks < (uint64_t)grid ? blocks : (uint64_t)grid)), b((unsigned)block);
    switch (tier) {
        case rtk::TIER_BASIC: hipLaunchKernelGGL(rtk::rt_scatter_kernel<rtk::TIER_BASIC>, g, b, 0, stream, P); break;
        case rtk::TIER_MESH: hipLaunchKernelGGL(rtk::rt_scatter_kernel<rtk::TIER_MESH>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL: hipLaunchKernelGGL(rtk::rt_scatter_kernel<rtk::TIER_FULL>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL_FLAT: hipLaunchKernelGGL(rtk::rt_scatter_kernel<rtk::TIER_FULL_FLAT>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL_GL: hipLaunchKernelGGL(rtk::rt_scatter_kernel<rtk::TIER_FULL_GL>, g, b, 0, stream, P); break;
        case rtk::TIER_FULL_DS: hipLaunchKernelGGL(rtk::rt_scatter_kernel<rtk::TIER_FULL_DS>, g, b, 0, stream, P); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
