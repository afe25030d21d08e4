// rt_path_entry.h -- the host entry points of the path kernel's tiers.
// rt_kernel_path.hip defines them, one object per tier in the product build;
// rt_kernel_common.hip (rtk_launch_frame, rtk_path_kernel_occupancy) calls
// them.  Both include this header, so a mismatch does not compile.
#pragma once
#include <hip/hip_runtime.h>

namespace rtk {
struct KParams;
}

extern "C" hipError_t rtk_launch_path_0(int, hipStream_t, const rtk::KParams*);
extern "C" hipError_t rtk_launch_path_0w(int, hipStream_t, const rtk::KParams*);
extern "C" hipError_t rtk_launch_path_1(int, hipStream_t, const rtk::KParams*);
extern "C" hipError_t rtk_launch_path_2(int, hipStream_t, const rtk::KParams*);
extern "C" hipError_t rtk_launch_path_3(int, hipStream_t, const rtk::KParams*);
extern "C" hipError_t rtk_launch_path_4(int, hipStream_t, const rtk::KParams*);
extern "C" hipError_t rtk_launch_path_5(int, hipStream_t, const rtk::KParams*);
extern "C" int rtk_occupancy_0(int*);
extern "C" int rtk_occupancy_1(int*);
extern "C" int rtk_occupancy_2(int*);
extern "C" int rtk_occupancy_3(int*);
extern "C" int rtk_occupancy_4(int*);
extern "C" int rtk_occupancy_5(int*);
