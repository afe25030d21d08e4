// rt_kernel.hip -- the persistent-threads f64 path-tracing megakernel for gfx950.
//
// One launch renders one frame (or one shard of rows) of Camera::render
// (src/camera.rs:161-202).  Work item = (pixel, stratum row s_i): the lane
// traces the sqrt_spp samples s_j of that row (camera.rs:183-192) one after
// another and stores their f64 sum; rt_reduce sums the rows of a pixel in s_i
// order and scales by pixel_sample_scale (camera.rs:193).
//
// ray_color's recursion (camera.rs:275-325) is run as a loop that carries a
// path throughput `beta` and radiance `L`; a lane whose path ends starts the
// next sample of its row at once, and a lane whose row ends takes the next row
// from a device-wide counter.  Refills are aggregated per wave: __ballot of the
// lanes that need work, one atomicAdd by the first of them, and each lane's
// slot from its mbcnt rank -- the wave64 prefix-sum compaction that keeps all
// 64 lanes tracing until the queue is empty.
//
// world.hit (hits.rs:34, bvh.rs:57, shapes.rs:88, volume.rs:37) is an explicit
// depth-first walk over the flattened world (rt_layout.h) with a per-lane stack
// in LDS, laid out [depth][lane] so a wave's pushes/pops hit 64 distinct banks.
//
// The device code, by subject, in the order the path unit includes it:
//   rt_builds.h   what the diag, trace and check builds add
//   rt_frame.h    Frame, KParams: the launch parameters
//   rt_texture.h  Texture::value, the sky gradient
//   rt_geom.h     Ray, the exact sphere / planar tests, Transform, HitInfo
//   rt_stack.h    the per-lane stacks, walk words, pops
//   rt_walk.h     Trav, trace_step, the media, a kernel's walk LDS set-up
//   rt_walk4.h    the 4-wide node visits, trace4_step (basic tier)
//   rt_record.h   make_record;  rt_lights.h  the lights' pdf_value / random
//   rt_shade.h    shade, shade_hit_basic
//   rt_scatter.h  scatter_level: one level handed back (the scatter unit only)
// beside the headers the CPU tests compile too (rt_slab.h, rt_sort4.h, ...).
//
// This file is the whole build (the check library, whose kernels share one
// g_check, and the A/B libraries): the seven units.  The product library
// compiles each as an object of its own, the path kernel's once per tier.
#include "rt_kernel_path.hip"
#include "rt_kernel_hit.hip"
#include "rt_kernel_occl.hip"
#include "rt_kernel_radiance.hip"
#include "rt_kernel_lights.hip"
#include "rt_kernel_scatter.hip"
#include "rt_kernel_common.hip"
