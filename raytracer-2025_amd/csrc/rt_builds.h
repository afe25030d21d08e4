// rt_builds.h -- what the variant builds add to the device code: the diag
// build's counters, the ISA marks, the trace build's globals and the check
// build's ref check.  The product build compiles all of it away.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_kernel.h"

namespace rtk {

// Diagnostic build (-DRT_DIAG, librt_mi355x_diag.so only): per-wave cycle
// stamps and per-lane work counters, summed into g_diag.  The product build
// compiles all of it away.
struct Diag {
#ifdef RT_DIAG
    unsigned long long cyc_refill = 0, cyc_trace = 0, cyc_shade = 0, cyc_media = 0;
    // basic / mesh tiers' unified loop: the parts of cyc_refill after the walk
    unsigned long long cyc_miss = 0, cyc_queue = 0, cyc_draws = 0;
    unsigned long long wave_trace_iters = 0, lane_trace_iters = 0, node_visits = 0, sphere_tests = 0, main_iters = 0;
    unsigned long long load_cyc = 0, loads = 0;  // -DRT_DIAG_LOADLAT: node-load latency (first active lane)
    unsigned long long pops = 0, pop_reads = 0;  // basic tier: pops and the stack entries they read
    unsigned long long big_tests = 0, big_hits = 0;  // basic tier: exact tests of spheres with r > 100 (and hits)
    // mesh / full tiers' unified walk-step loads: wave steps, steps whose
    // active lanes all read one record (of them node records), active lanes,
    // lanes reading the first active lane's record
    unsigned long long u_steps = 0, u_uniform = 0, u_uniform_node = 0, u_active = 0, u_same = 0;
    // ... steps whose active lanes all read nodes of the top 5 / 21 / 85 / 341
    // (rth::bvh4_convert numbers the top levels first, breadth-first), and
    // node reads of lanes at those nodes (lane counts)
    unsigned long long u_top[4] = {0, 0, 0, 0}, l_top[4] = {0, 0, 0, 0}, l_node = 0;
    // full tiers' shading rounds: rounds, lanes shaded, distinct shading
    // classes per round (miss, Lambertian by texture kind, Metal, Dielectric,
    // light, Isotropic, other) -- the branches a round executes one after the
    // other whatever the order of its lanes
    unsigned long long sh_rounds = 0, sh_lanes = 0, sh_classes = 0;
    // basic tier: wave iterations with no lane able to walk a node (pure
    // sphere rounds), and the lanes with a queued sphere in them
    unsigned long long pure_rounds = 0, pure_lanes = 0, pure_max_pn = 0;
    // ... per shading class (the 11 above): rounds in which it is present,
    // and its lanes
    unsigned long long cls_rounds[11] = {}, cls_lanes[11] = {};
    // basic tier, batch variant: the wave cycles of the camera stage (camera
    // draws, camera ray, candidate tests), the primary rays resolved from
    // the candidate table and the exact tests they ran
    unsigned long long cyc_camera = 0, prim_rays = 0, prim_tests = 0;
#endif
};
#ifdef RT_DIAG
constexpr int RT_DIAG_N = 64;
__device__ unsigned long long g_diag[RT_DIAG_N];
#define RT_DIAG_ONLY(x) x
#else
#define RT_DIAG_ONLY(x)
#endif
// ISA attribution build only (scripts/isa_phases.py, -DRT_ISA_MARKS): an
// assembler comment at each phase boundary of the basic tier's loop, so that
// the static instruction mix of every phase can be read off the ISA
#ifdef RT_ISA_MARKS
#define RT_ISA_MARK(name) asm volatile(";@@phase " name)
#else
#define RT_ISA_MARK(name)
#endif

#ifdef RT_WAVE_TRACE
// trace build: per lane of the grid, {start, end (s_memrealtime, 100 MHz),
// queue entries taken, rays traced, time / queue entry / rays so far at the
// lane's last refill, s_memtime ticks from start to end} (scripts/lane_trace.py)
constexpr uint32_t RT_TRACE_LANES = 1u << 19, RT_TRACE_W = 12;
__device__ unsigned long long g_lane_trace[RT_TRACE_LANES * RT_TRACE_W];
// ... and the rays begun per 0.25 ms of the launch (each wave's own clock
// from its start; one atomic per wave and bucket): the launch's throughput
// over time -- its ramp, steady state and drain
constexpr uint32_t RT_HIST_N = 1024, RT_HIST_TICKS = 25000;  // s_memrealtime: 100 MHz
__device__ unsigned long long g_ray_hist[RT_HIST_N];
struct RayHist {
    unsigned long long t0;
    uint32_t bucket = 0, count = 0;
    // beg: the lanes of the wave beginning a ray now (wave-uniform)
    __device__ __forceinline__ void add(unsigned long long beg) {
        const uint32_t b = min((uint32_t)((__builtin_amdgcn_s_memrealtime() - t0) / RT_HIST_TICKS), RT_HIST_N - 1);
        if (b != bucket) {
            flush();
            bucket = b;
        }
        count += (uint32_t)__popcll(beg);
    }
    __device__ __forceinline__ void flush() {
        if (count && __lane_id() == (uint32_t)(__ffsll((long long)__ballot(true)) - 1))
            atomicAdd(&g_ray_hist[bucket], (unsigned long long)count);
        count = 0;
    }
};
#endif

// ------------------------------------------------------------------ check build
// make check (-DRT_CHECK, librt_mi355x_check.so): every ref the walk, the
// hit record and the lights decode is checked against the count of its
// kind's array (SceneView::n_ref); a ref past its array is counted in
// g_check (the host's wait() turns a nonzero count into an error naming the
// first bad ref) and read as index 0, so the run itself stays in bounds.
// The product build compiles the check away.
#ifdef RT_CHECK
// The basic tier's slab guard (visit4_rows) reports through the same counter
// under a kind no ref has: "kind 15, index <node>" in the host's message is
// a node whose visit saw slab_f and slab_sorted_f differ, not a ref past its
// array.
constexpr uint32_t K_CHECK_SLAB = 15;
static_assert(K_CHECK_SLAB > K_POPXF, "the slab guard's marker must not be a ref kind");
// The basic tier's primary-ray guard (rt_kernel_path.hip: a camera ray resolved
// from its pixel's candidates is also walked) likewise: "kind 14, index
// <pixel>" is a pixel whose walk found another hit, or another t, than the
// candidate tests.
constexpr uint32_t K_CHECK_PRIMARY = 14;
static_assert(K_CHECK_PRIMARY > K_POPXF, "the primary-ray guard's marker must not be a ref kind");
__device__ unsigned long long g_check[2];
__device__ __noinline__ void check_fail(uint32_t ref) {
    atomicAdd(&g_check[0], 1ull);
    atomicCAS(&g_check[1], 0ull, (1ull << 32) | ref);
}
#endif
__device__ __forceinline__ uint32_t ref_idx(const SceneView& S, uint32_t ref) {
    const uint32_t i = ref_index(ref);
#ifdef RT_CHECK
    const uint32_t k = ref_kind(ref);
    if (k != K_NONE && i >= S.n_ref[k]) {
        check_fail(ref);
        return 0u;
    }
#endif
    return i;
}
// a planar run's last record (DBoxF::run) must lie inside planars too
__device__ __forceinline__ void check_run(const SceneView& S, uint32_t first, uint32_t n) {
#ifdef RT_CHECK
    if (n && first + n > S.n_ref[K_QUAD]) check_fail(make_ref(K_QUAD, first + n - 1));
#endif
}

}  // namespace rtk
