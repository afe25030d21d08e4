// rt_kernel_path.hip -- the host entry points of the path kernel's tiers.
// The product library compiles this unit once per tier (-DRT_TIER=N, each
// object with its own code-generation flags: raytracer-2025_amd/Makefile);
// with RT_TIER undefined it instantiates all five tiers and the basic tier's
// wide variant (the whole build, rt_kernel.hip).  The trace, check and diag
// builds' readers live here, with the kernels that write what they read.
#include "rt_kernel.hip"
#include "rt_path_entry.h"

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
