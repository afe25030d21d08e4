/* include/rt_mi355x.h -- C ABI of librt_mi355x.so, the MI355X (gfx950) render
 * path for caidj0/Raytracer-2025.
 *
 * The reference path is `Camera::render(&mut self, world: &dyn Hittable,
 * lights: Option<&dyn Hittable>) -> RgbImage` (src/camera.rs:161) over the
 * plugin traits Hittable (src/hit.rs:46-60), Material (src/material.rs:23-34),
 * Texture (src/texture.rs:5-7) and PDF (src/pdf.rs:13-16).  Rust trait objects
 * cannot cross a C boundary, so the world is described by constructor calls
 * that mirror the reference constructors one-to-one (each cited below), and is
 * flattened once into device arrays at the first rt_render that uses it.
 *
 * Conventions
 *  - Every constructor returns a handle >= 0 or a negative RT_E* code; the
 *    message of the last failure on this thread is rt_last_error().
 *  - Handles are per scene and per kind (texture / material / object).
 *    Textures and materials are shared (Arc in the reference): a handle may be
 *    used any number of times.  Objects are owned (Box<dyn Hittable>): passing
 *    an object to rt_hittables_add / rt_bvh_new / rt_transform_new /
 *    rt_constant_medium_new moves it, and a moved handle is RT_EMOVED
 *    afterwards (the Rust compiler rejects such reuse).
 *  - Reference panics (assert!, expect, unwrap, unimplemented!) become
 *    RT_EPANIC with a message; the library never aborts the process.
 *  - Not thread-safe per scene: calls on one scene are serialised by the
 *    caller.  Different scenes may be used from different threads, also
 *    when they render on the same device list or through the same rt_comm:
 *    the frame gathers of such renders are enqueued one whole RCCL group
 *    at a time.
 */
#ifndef RT_MI355X_H
#define RT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 3

enum rt_status {
    RT_OK = 0,
    RT_EINVAL = -1,       /* bad argument (null pointer, non-finite, out of range) */
    RT_EHANDLE = -2,      /* unknown handle or wrong kind */
    RT_EMOVED = -3,       /* object handle already moved into another object */
    RT_EDEGENERATE = -4,  /* Triangle::new returned None (triangle.rs:29-31) */
    RT_EPANIC = -5,       /* a reference panic condition was hit (message in rt_last_error) */
    RT_EUNSUPPORTED = -6, /* construct valid in the reference but not on this path yet */
    RT_EDEVICE = -7,      /* HIP runtime error, or no gfx950 device */
    RT_ENOMEM = -8,       /* host or device allocation failed */
    RT_ESTACK = -9        /* world deeper than the kernel's traversal stack */
};

typedef struct rt_scene rt_scene;

int32_t rt_abi_version(void);
const char* rt_last_error(void);
rt_scene* rt_scene_create(void);
void rt_scene_destroy(rt_scene* s);

/* ---- Textures (src/texture.rs) ------------------------------------------ */
/* SolidColor::new (texture.rs:14-16) */
int32_t rt_tex_solid(rt_scene* s, const double rgb[3]);
/* CheckerTexture::new (texture.rs:46-56) */
int32_t rt_tex_checker(rt_scene* s, double scale, int32_t even_tex, int32_t odd_tex);
/* ImageTexture::new / new_raw_image (texture.rs:82-97): pixels already decoded
 * to linear RGBA f32, row 0 = top (image.rs:63-82).  width == height == 0 is a
 * missing file: value() is cyan (texture.rs:167-169).  linear_interp selects
 * ImageInterpMethod::Linear (new_raw_image) instead of None. */
int32_t rt_tex_image(rt_scene* s, uint32_t width, uint32_t height, const float* rgba, int32_t linear_interp);
/* ImageTexture::new / new_raw_image (texture.rs:82-97) with the file path
 * given directly (the reference joins RTW_IMAGES or ./assets, image.rs:21-46):
 * the format comes from the extension as ImageReader::open takes it; the
 * library decodes PNG, JPEG and Radiance HDR (rt_image.hpp: the image crate's
 * into_rgba32f, then the sRGB EOTF unless raw or HDR, image.rs:63-82).  A file
 * that is missing, has no image extension, fails to decode or whose decoded
 * buffer would pass the image crate's default 512 MiB allocation limit
 * (ImageReader::decode reserves it first) is the reference's Image::EMPTY
 * (cyan); another image format (GIF, EXR, ...), a CMYK / arithmetic-coded /
 * 12-bit JPEG, or a file within the crate's limit but past this library's
 * 2^28 pixels is RT_EUNSUPPORTED.  raw != 0: no sRGB
 * conversion (new_raw_image); linear_interp selects ImageInterpMethod::Linear. */
int32_t rt_tex_image_file(rt_scene* s, const char* path, int32_t raw, int32_t linear_interp);
/* NoiseTexture::new (texture.rs:183-188).  Perlin tables are drawn from
 * SplitMix64(seed) in the order of perlin.rs:16-36. */
int32_t rt_tex_noise(rt_scene* s, double scale, uint64_t seed);
/* Book-1 sky: a user Texture for Camera.background (camera.rs:50) with
 * value(u,v,p) = (1-a)*horizon + a*zenith, a = (p.y+1)/2, p = unit direction
 * (environment.rs:14-24).  Not a reference type: the reference has no book-1
 * sky, so the build defines it through the Texture trait. */
int32_t rt_tex_sky_gradient(rt_scene* s, const double horizon[3], const double zenith[3]);

/* ---- Materials (src/material.rs) ---------------------------------------- */
int32_t rt_mat_empty(rt_scene* s);                                         /* EmptyMaterial 36-47 */
int32_t rt_mat_lambertian(rt_scene* s, int32_t tex);                       /* Lambertian::new 53-57 */
int32_t rt_mat_metal(rt_scene* s, const double albedo[3], double fuzz);   /* Metal::new 73-80 */
int32_t rt_mat_dielectric(rt_scene* s, int32_t tex, double ior);          /* Dielectric::new 103-108 */
/* DiffuseLight::new / new_with_material (152-169); inner_mat -1 = None */
int32_t rt_mat_diffuse_light(rt_scene* s, int32_t tex, int32_t inner_mat);
int32_t rt_mat_isotropic(rt_scene* s, int32_t tex);                        /* Isotropic::new 193-197 */
int32_t rt_mat_transparent(rt_scene* s);                                   /* Transparent 209-218 */
int32_t rt_mat_mix(rt_scene* s, int32_t mat1, int32_t mat2, double ratio); /* Mix::new 227-233 */
/* Mix::from_image (material.rs:235-247): ratio = the image texture's alpha at
 * (u, v) (ImageTexture::alpha, texture.rs:99-106: 1 for a missing image) */
int32_t rt_mat_mix_image(rt_scene* s, int32_t mat1, int32_t mat2, int32_t image_tex);
/* DisneyParameters (material/disney.rs:17-34) without base_color */
typedef struct rt_disney_params {
    uint32_t struct_size; /* sizeof(rt_disney_params) as the caller compiled it; as
                           * rt_render_opts: fields are only ever appended */
    int32_t thin;
    double roughness, anisotropic, sheen, sheen_tint, clearcoat, clearcoat_gloss, specular_tint, metallic, ior, flatness,
        spec_trans, diff_trans;
} rt_disney_params;
/* DisneyParameters::default (disney.rs:36-55) */
void rt_disney_params_default(rt_disney_params* params);
/* Disney { param_fn: |u, v, p| DisneyParameters { base_color: tex.value(u, v, p), ..params } }
 * (disney.rs:59-61): Disney::builder()...build() with a SolidColor, and the
 * closure of obj.rs:279-292 with any texture.  RT_EHANDLE: unknown texture;
 * RT_EINVAL: null pointer, a struct_size below this version's, a non-finite
 * field.  Ranges are not checked, as the reference checks none: a parameter
 * set that makes NaNs is counted in rt_stats.panics like every other
 * reference assert. */
int32_t rt_mat_disney(rt_scene* s, int32_t base_color_tex, const rt_disney_params* params);
/* Portal::new(attenuation, position_offset, rotation) (material/portal.rs:15-25):
 * scatter is ScatterRecord::Ray((attenuation, Ray::new_with_time(rec.p +
 * position_offset, rotation.rotate_vector(r_in.direction), r_in.time))), so a
 * hit costs no draw and takes no light sampling (camera.rs:317-319); emitted is
 * black.  Null offset3 = zero, null quat_wxyz = the identity, as
 * rt_transform_new's nulls.  RT_EINVAL: a null scene, a null attenuation, any
 * non-finite value.  Nothing else is checked, as the reference checks nothing:
 * the quaternion is used as given -- a zero or non-unit one is accepted and is
 * not normalised, nor is the rotated direction -- and a direction that cannot
 * be normalised downstream is counted in rt_stats.panics like every other
 * reference expect. */
int32_t rt_mat_portal(rt_scene* s, const double attenuation[3], const double* offset3, const double* quat_wxyz);

/* ---- Hittables ------------------------------------------------------------ */
/* Sphere::new (shapes/sphere.rs:25-35) */
int32_t rt_sphere(rt_scene* s, const double center[3], double radius, int32_t mat);
/* Sphere::new_with_motion (shapes/sphere.rs:37-51) */
int32_t rt_sphere_moving(rt_scene* s, const double center1[3], const double center2[3], double radius, int32_t mat);
/* Quad::new (shapes/quad.rs:30-47) */
int32_t rt_quad(rt_scene* s, const double anchor[3], const double u[3], const double v[3], int32_t mat);
/* Triangle::new (shapes/triangle.rs:28-46); RT_EDEGENERATE where it returns None */
int32_t rt_triangle(rt_scene* s, const double anchor[3], const double u[3], const double v[3], int32_t mat);
/* Hittables::default (hits.rs:9) -- an empty list object */
int32_t rt_hittables_new(rt_scene* s);
/* Hittables::add (hits.rs:27-30); moves `object` */
int32_t rt_hittables_add(rt_scene* s, int32_t list, int32_t object);
/* BVH::new(Hittables) (bvh.rs:12-46); moves `list`.  The reference topology is
 * built; rendering rebuilds it with a binned SAH unless RT_FLAG_REFERENCE_BVH. */
int32_t rt_bvh_new(rt_scene* s, int32_t list);
/* build_box (shapes/quad.rs:128-189); returns a Hittables object */
int32_t rt_build_box(rt_scene* s, const double a[3], const double b[3], int32_t mat);
/* Transform::new (shapes.rs:31-47); moves `object`; null pointers = None
 * (offset 0, identity quaternion (w,x,y,z), scale 1) */
int32_t rt_transform_new(rt_scene* s, int32_t object, const double* offset3, const double* quat_wxyz, const double* scale3);
/* ConstantMedium::new_with_tex (volume.rs:23-33); moves `boundary` */
int32_t rt_constant_medium_new(rt_scene* s, int32_t boundary, double density, int32_t tex);
/* Wavefont::new (shapes/obj.rs:117-134) with the OBJ path given directly (the
 * reference joins RTW_OBJS or ./assets, prefix and file name, obj.rs:86-115;
 * MTL and map_* paths resolve against the OBJ's directory).  tobj
 * GPU_LOAD_OPTIONS semantics; one BVH per loaded model, each triangle under a
 * RemappedMaterial (vertex normals + texture coordinates, obj.rs:20-81).
 * vanilla != 0: Metal / Dielectric from Pm / Tf (obj.rs:289-298); image maps
 * (map_Kd, map_Ke, map_d, map_Bump / normal) are decoded as rt_tex_image_file
 * does (obj.rs:212-345: map_d -> Mix::from_image(Transparent, mat)); Disney
 * materials -> RT_EUNSUPPORTED.  Returns a Hittables object (possibly empty).
 * rt_wavefront_load_flags(.., RT_OBJ_DISNEY) builds the Disney materials. */
int32_t rt_wavefront_load(rt_scene* s, const char* obj_path, int32_t vanilla);
/* Wavefont::new in full.  flags:
 *   RT_OBJ_VANILLA  Wavefont::new's vanilla_material: Metal where Pm == 1,
 *                   Dielectric where the mean of Tf == 1 (obj.rs:271-278)
 *   RT_OBJ_DISNEY   every other material is the Disney of obj.rs:279-292:
 *                   rt_mat_disney(base, params), base the texture the other
 *                   arms use (map_Kd, else Kd), params rt_disney_params_default
 *                   with roughness = Pr (0.5 when absent), anisotropic = aniso
 *                   (0), sheen = Ps (0), metallic = Pm (0), clearcoat = Pc (0),
 *                   clearcoat_gloss = Pcr (0), ior = Ni (1.45), spec_trans =
 *                   the mean of Tf's numbers (0); a value that does not parse
 *                   as str::parse::<f64> takes the default.  Ke, map_Ke, map_d,
 *                   d and the normal map wrap it as they wrap the other arms.
 * Without RT_OBJ_DISNEY such a material is refused as rt_wavefront_load
 * refuses it (callers of ABI 3 rely on that): rt_wavefront_load(s, p, vanilla)
 * is rt_wavefront_load_flags(s, p, vanilla ? RT_OBJ_VANILLA : 0).
 * A Disney parameter that comes out non-finite (`Tf` without a number is
 * 0 / 0, `Pr nan`) makes the reference render NaNs and rt_mat_disney refuses
 * it: the load is RT_EUNSUPPORTED, and rt_last_error names the material and
 * the MTL key.  Unknown flag bits: RT_EINVAL.  Everything else (paths, missing
 * files, panics, ownership) as rt_wavefront_load. */
#define RT_OBJ_VANILLA 1u /* Wavefont::new's vanilla_material */
#define RT_OBJ_DISNEY 2u  /* build obj.rs:279-292's Disney where rt_wavefront_load refuses */
int32_t rt_wavefront_load_flags(rt_scene* s, const char* obj_path, uint32_t flags);

/* Quaternion::from_axis_angle / from_euler (utils/quaternion.rs:23-53), host helpers */
int32_t rt_quat_from_axis_angle(const double axis[3], double angle_degrees, double out_wxyz[4]);
void rt_quat_from_euler(double yaw, double pitch, double roll, double out_wxyz[4]);

/* ---- Camera (src/camera.rs:45-61 pub fields) ------------------------------ */
typedef struct rt_camera {
    double aspect_ratio;
    uint32_t image_width;
    uint32_t samples_per_pixel; /* traced samples = floor(sqrt(spp))^2 (camera.rs:212) */
    uint32_t max_depth;
    int32_t background_tex; /* Environment texture; -1 = SolidColor(BLACK) (camera.rs:83-85) */
    double vertical_fov_in_degrees;
    double look_from[3];
    double look_at[3];
    double vec_up[3];
    double defocus_angle_in_degrees;
    double focus_distance;
    int32_t toon_map; /* 0 = ToonMap::None, 1 = ToonMap::ACES (utils/color.rs:8-11) */
    int32_t reserved;
} rt_camera;

/* Camera::default (camera.rs:76-104) */
void rt_camera_default(rt_camera* cam);
/* Camera::initilize's image_height (camera.rs:205-210) */
uint32_t rt_camera_image_height(const rt_camera* cam);

typedef struct rt_comm rt_comm;

typedef struct rt_render_opts {
    /* sizeof(rt_render_opts) of the caller's header, set by
     * rt_render_opts_default: the library reads a field only when the
     * caller's struct holds it, and refuses (RT_EINVAL) a size smaller than
     * ABI version 3's -- fields are only ever appended. */
    uint32_t struct_size;
    uint32_t reserved0;
    uint64_t seed;       /* render RNG key (oracle/rng_contract.hpp) */
    uint32_t row_offset; /* shard: render rows y = row_offset + k*row_stride */
    uint32_t row_stride; /* 0 or 1 = every row */
    uint32_t threads;    /* CPU implementations only; 0 = all cores */
    uint32_t flags;      /* RT_FLAG_* */
    void* stream;        /* hipStream_t for rt_render_device (of devices[0] when n_devices > 1); NULL = default */
    /* In-process multi-GPU (replaces the rayon pool, camera.rs:178-197):
     * n_devices > 1 renders the shard's rows interleaved over the HIP devices
     * devices[0..n_devices) -- part k takes the shard rows k, k + n, k + 2n,
     * ... -- one host thread per device (world flatten shared, one upload per
     * device), and gathers the parts onto devices[0] over RCCL (ncclSend /
     * ncclRecv in one group; peer copies when a device repeats in the list).
     * 0 or 1 = the calling thread's current device only. */
    uint32_t n_devices;
    uint32_t reserved;
    const int32_t* devices;
    /* Multi-process (one process per GPU): a communicator from rt_comm_init.
     * Rank r renders the shard rows r, r + nranks, ... on its current device;
     * rank 0 receives the whole shard (RCCL gather), other ranks' outputs are
     * not written.  Exclusive with n_devices > 1. */
    rt_comm* comm;
} rt_render_opts;

/* Keep the reference BVH topology (bvh.rs:16-46: longest axis, sort by box
 * min, median split) instead of the default binned-SAH rebuild of every BVH.
 * Closest-hit results agree up to exact ties in t; used for A/B measurement. */
#define RT_FLAG_REFERENCE_BVH 1u

void rt_render_opts_default(rt_render_opts* opts);

typedef struct rt_stats {
    uint64_t samples;         /* traced camera samples (pixels x floor(sqrt(spp))^2), all devices of this call */
    uint64_t rays;            /* ray_color calls that reached world.hit */
    uint64_t panics;          /* reference assert/expect conditions (NaN, zero pdf, ...) */
    uint64_t n_devices;       /* devices that rendered (1 per rank with a comm) */
    double render_ms;         /* wall time of the call (host) */
    double kernel_ms;         /* device time of the path-tracing kernel (HIP events), max over devices */
    double flatten_ms;        /* world flatten + upload, 0 when cached */
    double gather_ms;         /* device time of the framebuffer gather on devices[0] / rank 0, 0 without one */
} rt_stats;

/* Camera::render(&world, lights) (camera.rs:161-202).  world: object handle;
 * lights: object handle or -1 (None).  Writes the shard's rows, compact and
 * row-major (y down), as linear RGB f32 = pixel_color * pixel_sample_scale
 * (camera.rs:193) to out_linear_rgb (rows x W x 3, may be NULL) and as sRGB u8
 * = Color::to_rgb (utils/color.rs:27-36) to out_srgb (may be NULL).  Blocking.
 * Objects passed here are borrowed, not moved. */
int32_t rt_render(rt_scene* s, int32_t world, int32_t lights, const rt_camera* cam, const rt_render_opts* opts,
                  float* out_linear_rgb, uint8_t* out_srgb, rt_stats* stats);

/* What rt_render would upload for (world, lights): host-only, no device needed. */
typedef struct rt_world_info {
    uint64_t device_bytes;    /* size of the flattened world blob */
    uint32_t bvh_nodes;       /* 4-wide BVH nodes the kernel walks */
    uint32_t primitives;      /* spheres + moving spheres + quads + triangles */
    uint32_t bvh_leaves;      /* objects under BVHs */
    uint32_t stack_need;      /* traversal-stack entries one lane needs */
    uint32_t kernel_tier;     /* 0 = spheres/BVH/basic materials, 1 = + quads/triangles/OBJ, 2 = full,
                               * 3 = full without BVH nodes, 4 = full + general lights / nested
                               * wrapper materials, 5 = 4 + the Disney BSDF (rt_kernel.h Tier).
                               * A Portal material takes tier 4, or 5 beside a Disney material */
    uint32_t features;        /* F_* bits (rt_layout.h); 2048 = F_PORTAL: a Portal material is reachable */
} rt_world_info;
int32_t rt_world_info_get(rt_scene* s, int32_t world, int32_t lights, int32_t background_tex, uint32_t flags,
                          rt_world_info* out);

/* ---- Hit queries: Hittable::hit (src/hit.rs:46-60) ------------------------- */
/* One query ray.  The direction is used as given (not normalised); t_max is
 * the interval's upper end and may be +inf. */
typedef struct rt_ray {
    double origin[3];
    double dir[3];
    double time;
    double t_max;
} rt_ray; /* 64 B */
/* HitRecord (hit.rs:11-43) as hit() returns it: p, the unit normal turned
 * against the ray, the primitive's own (u, v) -- for an OBJ triangle the
 * record before RemappedMaterial::remap_record (obj.rs:32-62), which belongs
 * to the material -- and mat, the index in the flattened material table (the
 * rt_mat_* handle of a material the caller made).  A ConstantMedium hit has
 * RT_HIT_MEDIUM, u = v = 0 and the normal (1, 0, 0) of volume.rs:67-72, which
 * HitRecord::new turns against the ray like any other: (-1, -0, -0) where
 * dir.x >= 0; its mat is the medium's own Isotropic, a slot of the table
 * that no caller's handle names.  A miss has flags 0, mat -1 and every
 * double 0. */
typedef struct rt_hit_record {
    double t;
    double p[3];
    double normal[3];
    double u, v;
    int32_t mat;
    uint32_t flags; /* RT_HIT_* */
} rt_hit_record;    /* 80 B */
#define RT_HIT_FOUND 1u
#define RT_HIT_FRONT_FACE 2u
#define RT_HIT_MEDIUM 4u
/* world.hit(Ray{origin, dir, time}, [1e-8, t_max]) (camera.rs:286 with the
 * caller's upper end; both ends inclusive, interval.rs:65-67) for each of n
 * rays, from host arrays into host arrays on the calling thread's current
 * device.  Blocking.  A ConstantMedium's one draw per test (volume.rs:58) is
 * the RNG contract's medium stream (oracle/rng_contract.hpp) of key `seed`,
 * pixel = the ray's index, sample 0, vertex 1 -- hence n < 2^32.  flags:
 * RT_FLAG_REFERENCE_BVH or 0.  The world is flattened and uploaded as for
 * rt_render(world, lights = -1, background = -1, flags) and shares the
 * scene's per-device world cache; the device work is ordered after the
 * scene's previous device work, as renders are.
 * RT_EINVAL: a null scene; a null array with n > 0; n >= 2^32; unknown flags;
 * a ray with a non-finite origin, direction or time, a zero direction, or a
 * NaN or negative t_max.  RT_EHANDLE / RT_EMOVED as rt_render.  RT_EDEVICE
 * without a gfx950 device (there is no CPU fallback).  n == 0 is RT_OK,
 * touches no device and needs no arrays. */
int32_t rt_world_hit(rt_scene* s, int32_t world, uint64_t seed, uint32_t flags, const rt_ray* rays, uint64_t n,
                     rt_hit_record* out);
/* The same from and to gfx950 device arrays, enqueued on `stream` (a
 * hipStream_t; NULL = the default stream) without waiting.  The rays cannot be
 * validated here: they are the caller's duty, and the kernel ends and writes a
 * record for any ray. */
int32_t rt_world_hit_device(rt_scene* s, int32_t world, uint64_t seed, uint32_t flags, const rt_ray* rays_device,
                            uint64_t n, rt_hit_record* out_device, void* stream);

/* ---- Occlusion queries: is anything in the way ----------------------------- */
/* world.hit(Ray{origin, dir, time}, [1e-8, t_max]).is_some() (hit.rs:46-60)
 * for each of n rays -- the any-hit query of shadow rays, visibility tests
 * and ambient occlusion, which need no record: the walk ends at the first
 * accepted hit and one byte a ray comes back.  The contract: for the same
 * (world, seed, flags, rays, index),
 *     out[i] == ((record[i].flags & RT_HIT_FOUND) != 0)
 * of rt_world_hit -- 1 or 0, nothing else.  A ConstantMedium hit occludes, as
 * hit returning Some does, and its draw is rt_world_hit's: the medium stream
 * of (seed, pixel = the ray's index, sample 0, vertex 1).
 * A segment test from a to b is the ray origin = a, dir = b - a with t_max
 * just under 1 (b itself, when it lies on a surface, is then not in the way):
 * that is what t_max is on the ray for.
 * Everything else is rt_world_hit's: the argument checks and error codes (the
 * host variant validates every ray), n == 0 (RT_OK, no device touched, no
 * arrays needed), n < 2^32, flags, the flattening and the scene's per-device
 * world cache -- a render, a hit query and an occlusion query of one
 * flattening upload it once -- and the ordering after the scene's previous
 * device work.  Host arrays, blocking: */
int32_t rt_world_occluded(rt_scene* s, int32_t world, uint64_t seed, uint32_t flags, const rt_ray* rays, uint64_t n,
                          uint8_t* out);
/* The same from and to gfx950 device arrays, enqueued on `stream` without
 * waiting, as rt_world_hit_device: the rays are the caller's duty, and the
 * kernel ends and writes a byte for any ray, and none past out_device[n - 1]. */
int32_t rt_world_occluded_device(rt_scene* s, int32_t world, uint64_t seed, uint32_t flags, const rt_ray* rays_device,
                                 uint64_t n, uint8_t* out_device, void* stream);

/* ---- Radiance queries: Camera::ray_color for caller-given rays ---------------- */
/* The shading half of the path, open to any ray: an orthographic, fisheye or
 * equirectangular view, a light probe, a lightmap texel, a re-trace of a few
 * pixels, a host-side integrator that wants the radiance along a ray. */
typedef struct rt_radiance_opts {
    uint32_t struct_size;   /* set by rt_radiance_opts_default; fields only ever appended */
    uint32_t max_depth;     /* Camera.max_depth; 0 -> every result BLACK (camera.rs:282-284) */
    uint64_t seed;          /* RNG key (oracle/rng_contract.hpp) */
    uint32_t samples;       /* ray_color evaluations per ray, >= 1 */
    uint32_t flags;         /* RT_FLAG_REFERENCE_BVH or 0 */
    int32_t background_tex; /* Camera.background; -1 = BLACK */
    uint32_t first_index;   /* RNG pixel of ray 0; ray i uses first_index + i */
    void* stream;           /* device variant only; NULL = default stream */
} rt_radiance_opts;
/* max_depth 10, samples 1, background_tex -1, everything else 0 */
void rt_radiance_opts_default(rt_radiance_opts* opts);

typedef struct rt_radiance {
    double rgb[3];   /* (sum over s of ray_color_s) * (1.0 / samples), f64 */
    uint32_t rays;   /* ray_color calls that reached world.hit, all samples */
    uint32_t panics; /* samples that met a reference assert / expect / NaN */
} rt_radiance;       /* 32 B */

/* For ray i of n and each sample s < opts->samples,
 *     Camera::ray_color(Ray{origin, dir, time}, max_depth, world, lights)
 * (camera.rs:275-325) with Camera.background = background_tex; the direction
 * is used as given (not normalised).  Over every world rt_render accepts:
 * lights, media, wrapper materials, Disney and Portal included.
 * RNG: the contract's main and medium streams (oracle/rng_contract.hpp) keyed
 * (seed, pixel = first_index + i, sample = s, vertex = k) for the k-th
 * ray_color call along the path, k >= 1 -- what rt_render draws from vertex 1
 * on; vertex 0 (the camera ray's draws) is not used.
 * The samples are summed in f64 in ascending s from zero and the sum is
 * multiplied once by 1.0 / samples: the result does not depend on scheduling.
 * t_max bounds the first world.hit only, the interval [1e-8, t_max] with both
 * ends inclusive: a first hit past it is a miss and the background is
 * returned; later vertices use [1e-8, inf), and t_max = +inf is plain
 * ray_color.
 * A sample that panics (a reference assert / expect, or a NaN result) ends
 * there and adds what rt_render would have added for it -- the radiance
 * gathered so far, or black if that is NaN (camera.rs:323) -- and counts once
 * in `panics`.
 * RT_EINVAL: a null scene or opts; a null array with n > 0; struct_size below
 * this version's; samples == 0; unknown flags; first_index + n > 2^32; (no
 * max_depth is refused: rt_render refuses none); in the host variant a ray
 * with a non-finite origin, direction or time, a zero direction, or a NaN or
 * negative t_max, named in rt_last_error as rt_world_hit names it.
 * RT_EHANDLE / RT_EMOVED / RT_EUNSUPPORTED / RT_ESTACK as rt_render gives them
 * for (world, lights, background_tex).  RT_EDEVICE without a gfx950 device
 * (there is no CPU fallback).  n == 0 is RT_OK, touches no device and needs
 * no arrays.  max_depth == 0 with n > 0 writes zeros without a kernel launch.
 * The world is flattened and uploaded as for rt_render(world, lights,
 * background_tex, flags) -- not as for rt_world_hit, whose flattening drops
 * what only materials need -- and shares the scene's per-device world cache
 * with renders: a render and a radiance query of one flattening upload once.
 * The device work is ordered after the scene's previous device work, as
 * renders are.  Host arrays, on the calling thread's current device,
 * blocking: */
int32_t rt_world_radiance(rt_scene* s, int32_t world, int32_t lights, const rt_radiance_opts* opts, const rt_ray* rays,
                          uint64_t n, rt_radiance* out);
/* The same from and to gfx950 device arrays, enqueued on opts->stream without
 * waiting (max_depth == 0: a memset).  The rays are the caller's duty, as in
 * rt_world_hit_device; the kernel ends and writes a record for any ray, and
 * none past out_device[n - 1]. */
int32_t rt_world_radiance_device(rt_scene* s, int32_t world, int32_t lights, const rt_radiance_opts* opts,
                                 const rt_ray* rays_device, uint64_t n, rt_radiance* out_device);

/* ---- Lights queries: Hittable::pdf_value and Hittable::random of the lights ---- */
/* The two Hittable methods (hit.rs:46-60) the reference's importance sampling
 * rests on, called through HittablePDF (pdf.rs:66-88) on the lights object at
 * every diffuse vertex (camera.rs:298-311), open to any batch of points: a
 * next-event-estimation vertex of a host-side integrator built on rt_world_hit
 * and rt_world_occluded, a light probe, a lightmap texel, a many-light study. */
typedef struct rt_lights_opts {
    uint32_t struct_size;   /* set by rt_lights_opts_default; fields only ever appended */
    uint32_t flags;         /* RT_FLAG_REFERENCE_BVH or 0 */
    uint64_t seed;          /* RNG key (rt_lights_sample only) */
    uint32_t samples;       /* rt_lights_sample: draws per origin, >= 1; rt_lights_pdf ignores it */
    uint32_t first_index;   /* RNG pixel of origin 0; origin i uses first_index + i */
    int32_t background_tex; /* only selects the flattening, see below; -1 = BLACK */
    uint32_t reserved;
    void* stream;           /* device variants only; NULL = default stream */
    uint64_t reserved1;     /* room for a later version's field; not read */
} rt_lights_opts;           /* 48 B */
/* samples 1, background_tex -1, everything else 0 */
void rt_lights_opts_default(rt_lights_opts* opts);

typedef struct rt_light_sample {
    double dir[3];   /* lights.random(origin): a unit vector */
    double pdf;      /* lights.pdf_value(origin, dir): HittablePDF::value of that draw */
    uint32_t flags;  /* RT_LIGHT_PANIC */
    uint32_t reserved;
} rt_light_sample;   /* 40 B */
#define RT_LIGHT_PANIC 1u

/* rt_lights_pdf: out[i] = lights.pdf_value(origin_i, dir_i) for i < n; origins3
 * and dirs3 are n packed triples of doubles.  Quad::pdf_value quad.rs:108-120
 * (Triangle likewise), Sphere::pdf_value sphere.rs:114-132, Hittables::pdf_value
 * hits.rs:52-67 (the children's values summed in order, over their count),
 * Transform::pdf_value shapes.rs:117-123.  The direction is used as given (not
 * normalised).  The reference makes the ray with Ray::new at time 0
 * (ray.rs:11-17), so a moving sphere is taken at center.at(0); the interval
 * tested is [1e-8, inf).  The value is returned as computed: a direction that
 * misses every light gives 0, and where the arithmetic gives NaN, NaN is
 * returned -- there Hittables::pdf_value panics with "The sum of pdf is NaN!"
 * (hits.rs:52-67) and ray_color's own check panics (camera.rs:323);
 * pdf_value has no other panic.
 *
 * rt_lights_sample: out[i * samples + s] is draw s for origin i:
 * dir = lights.random(origin_i) (Hittables::random hits.rs:69-75,
 * Quad quad.rs:122-125, Triangle triangle.rs:117-128, Sphere sphere.rs:134-144,
 * Transform shapes.rs:125-132) and pdf = lights.pdf_value(origin_i, dir).
 * RNG: the contract's main stream (oracle/rng_contract.hpp) keyed (seed,
 * pixel = first_index + i, sample = s, vertex = 1), slots 0, 1, 2, ... in the
 * order random draws them: a list's child choice first at each list level,
 * then the primitive's two (the deepest accepted tree draws 6, under the
 * contract's 16).  A draw panics when one of random's expects fails -- a
 * direction that cannot be normalised, as from an origin at a sphere light's
 * centre: such a draw has flags = RT_LIGHT_PANIC, dir = 0 and pdf = 0.  A NaN
 * pdf on a good direction is returned as NaN without the flag, as in
 * rt_lights_pdf.  A result depends on (seed, first_index + i, s) alone, never
 * on scheduling or on the batch's size.
 *
 * world, lights, flags and background_tex name the flattening: the world is
 * flattened and uploaded exactly as for rt_render(world, lights,
 * background_tex, flags) and shares the scene's per-device world cache, so a
 * render, a radiance query and a lights query of one flattening upload once.
 * lights.pdf_value does not need the world; it is an argument because the
 * cache holds one flattening per scene and device, and a lights-only
 * flattening would evict a million-triangle world between a hit query and the
 * light sample that follows it.  Every lights object rt_render accepts is
 * accepted and every one it refuses is refused with rt_render's code and
 * message (a BVH or a ConstantMedium among the lights, or an empty list:
 * RT_EPANIC; a tree deeper than 4 levels: RT_EUNSUPPORTED).  lights = -1 is
 * RT_EINVAL: `lights: None` has nothing to sample.
 *
 * RT_EINVAL: a null scene or opts; struct_size below this version's;
 * samples == 0 (rt_lights_sample); unknown flags; first_index + n > 2^32;
 * n * samples >= 2^40; a null array with n > 0; in the host variants a
 * non-finite origin or (rt_lights_pdf) a non-finite or zero direction, named
 * in rt_last_error by its index as rt_world_hit names a ray.  RT_EHANDLE /
 * RT_EMOVED as rt_render gives them.  RT_EDEVICE without a gfx950 device
 * (there is no CPU fallback).  n == 0 is RT_OK, touches no device and needs
 * no arrays.  The device work is ordered after the scene's previous device
 * work, as the other queries' is.  Host arrays, on the calling thread's
 * current device, blocking: */
int32_t rt_lights_pdf(rt_scene* s, int32_t world, int32_t lights, const rt_lights_opts* opts, const double* origins3,
                      const double* dirs3, uint64_t n, double* out);
int32_t rt_lights_sample(rt_scene* s, int32_t world, int32_t lights, const rt_lights_opts* opts, const double* origins3,
                         uint64_t n, rt_light_sample* out);
/* The same from and to gfx950 device arrays, enqueued on opts->stream without
 * waiting.  The arrays are the caller's duty, as in rt_world_hit_device; the
 * kernel ends and writes an output for any input, and none past out_device[n - 1]
 * (rt_lights_sample_device: out_device[n * samples - 1]). */
int32_t rt_lights_pdf_device(rt_scene* s, int32_t world, int32_t lights, const rt_lights_opts* opts,
                             const double* origins3_device, const double* dirs3_device, uint64_t n, double* out_device);
int32_t rt_lights_sample_device(rt_scene* s, int32_t world, int32_t lights, const rt_lights_opts* opts,
                                const double* origins3_device, uint64_t n, rt_light_sample* out_device);

/* ---- Scatter queries: Material::emitted / ::scatter and the PDF behind it ----- */
/* One ray_color level (camera.rs:286-316) for caller-given rays, without the
 * recursion and without the lights mix: what the surface a ray meets emits,
 * how it scatters, and the BSDF and density of a direction the caller drew
 * elsewhere (towards a light: rt_lights_sample).  With rt_lights_* and
 * rt_world_occluded the caller owns the integrator's loop -- next-event
 * estimation, MIS, Russian roulette, path guiding, first-hit AOVs -- while
 * every bounce runs on the library's walk and its materials: textures, Mix /
 * DiffuseLight wrappers, OBJ RemappedMaterials, Disney and Portal included.
 * The query takes rays, not hit records: an OBJ triangle's material needs the
 * primitive (remap_record, obj.rs:32-62), and no caller-given index is read. */
typedef struct rt_scatter_opts {
    uint32_t struct_size;   /* set by rt_scatter_opts_default; fields only ever appended */
    uint32_t flags;         /* RT_FLAG_REFERENCE_BVH or 0 */
    uint64_t seed;          /* RNG key (oracle/rng_contract.hpp) */
    uint32_t sample;        /* RNG sample coordinate of every ray of the call */
    uint32_t vertex;        /* RNG vertex coordinate, 1 <= vertex < 2^28: the k-th ray_color call of the caller's path */
    uint32_t first_index;   /* RNG pixel of ray i is first_index + i when `indices` is NULL */
    int32_t background_tex; /* Camera.background: what a miss returns; -1 = BLACK */
    void* stream;           /* device variant only; NULL = default stream */
    uint64_t reserved1;     /* not read */
} rt_scatter_opts;          /* 48 B */
/* vertex 1, background_tex -1, everything else 0 */
void rt_scatter_opts_default(rt_scatter_opts* opts);

typedef struct rt_scatter {
    rt_hit_record hit;  /* exactly rt_world_hit's record for this ray (before remap_record) */
    double emitted[3];  /* hit: rec.mat.emitted(r, rec); miss: Environment::value(r) */
    double f[3];        /* RT_SCATTER_RAY: the attenuation; RT_SCATTER_PDF: PDF::value(dir).0 */
    double pdf;         /* RT_SCATTER_PDF: PDF::value(dir).1 (may be 0: camera.rs:309 is the caller's assert); else 0 */
    double origin[3];   /* the scattered ray's origin (rec.p; Portal: rec.p + offset) */
    double dir[3];      /* RAY: skip_pdf_ray's direction as made (not normalised); PDF: PDF::generate() */
    double eval_f[3];   /* RT_SCATTER_EVAL: PDF::value(eval_dir).0 */
    double eval_pdf;    /* RT_SCATTER_EVAL: PDF::value(eval_dir).1 */
    uint32_t flags;     /* RT_SCATTER_* */
    uint32_t draws;     /* main-stream slots of this vertex the reference's code consumed */
} rt_scatter;           /* 224 B */
#define RT_SCATTER_RAY 1u       /* scatter returned ScatterRecord::Ray */
#define RT_SCATTER_PDF 2u       /* scatter returned ScatterRecord::PDF */
#define RT_SCATTER_NO_SAMPLE 4u /* with PDF: generate() returned None (Disney); dir, f, pdf are 0 */
#define RT_SCATTER_EVAL 8u      /* eval_f / eval_pdf hold PDF::value(eval_dir) */
#define RT_SCATTER_PANIC 16u    /* a reference unwrap / expect / assert of this level failed */

/* For ray i of n: world.hit(Ray{origin, dir, time}, [1e-8, t_max]) -- t_max is
 * the first-hit bound as in rt_world_radiance: a hit past it is a miss -- and
 * `hit` is bit for bit what rt_world_hit writes for that ray (its query-mode
 * (u, v) and mat, RT_HIT_MEDIUM and the medium's normal included).
 * A miss: `hit` is the miss record, emitted = Environment::value of
 * background_tex (black for -1), every other field 0, flags 0.
 * A hit: the shading record is the path kernels' -- remap_record with vertex
 * normals, texture coordinates and normal map for an OBJ triangle.  emitted =
 * Material::emitted through the wrapper tree (DiffuseLight, Mix), returned as
 * computed: a NaN is a NaN (the check of camera.rs:323 is ray_color's).  Then
 * Material::scatter through the wrappers, the Mix draws first:
 *   None (a light, Metal's `?`, a DiffuseLight without a material): neither
 *     kind bit; f, pdf, origin and dir are 0.
 *   ScatterRecord::Ray (Metal, Dielectric, Transparent, Portal):
 *     RT_SCATTER_RAY; f the attenuation, (origin, dir) the ray, pdf 0.
 *   ScatterRecord::PDF (CosinePDF, SpherePDF, DisneyPDF): RT_SCATTER_PDF;
 *     dir = generate(), (f, pdf) = value(dir), origin = rec.p.  A generate()
 *     that returns None (Disney) adds RT_SCATTER_NO_SAMPLE and leaves them 0.
 * There is no lights mix: no MixturePDF and no mixture draw.  The slots of the
 * vertex are the wrappers' draws, then the material's, then generate's, in
 * reference order, and `draws` counts them; the caller mixes with the lights
 * itself through rt_lights_*.  The scattered ray's time is the ray's own.
 * eval_dirs3, when not NULL, holds n packed triples: for an RT_SCATTER_PDF
 * record (eval_f, eval_pdf) = PDF::value(eval_dir_i) of the same PDF object --
 * the BSDF half of an MIS weight for a direction drawn from the lights -- and
 * RT_SCATTER_EVAL is set, whether or not generate() returned a direction; for
 * every other outcome the two fields are 0 and the bit is clear.
 * A panic of the level (remap_record's unwraps, unit() of the incoming
 * direction in Dielectric, the ONB / CosinePDF::value unwraps, Disney's panics,
 * more than 16 slots): flags == RT_SCATTER_PANIC alone, `hit` stays, every
 * other field 0.  pdf == 0 is not a panic here.
 * RNG: the contract's main and medium streams (oracle/rng_contract.hpp) keyed
 * (seed, pixel, sample, vertex) with pixel = indices[i], or first_index + i
 * when indices is NULL: a caller that compacts its live paths between bounces
 * keeps each path's stream by handing its pixel on.  A result depends on that
 * key, the ray and its eval direction alone, never on n or on scheduling.  So
 * in a world rendered without lights the query applied at vertex 1, 2, ...
 * with stable indices retraces the path rt_render / rt_world_radiance trace,
 * draw for draw, media included.
 * The world is flattened and uploaded as for rt_render(world, lights,
 * background_tex, flags) and shares the scene's per-device world cache;
 * `lights` only names the flattening (it may be -1) and is never sampled.  The
 * device work is ordered after the scene's previous device work, as
 * rt_world_radiance's is.
 * RT_EINVAL: a null scene or opts; struct_size below this version's; unknown
 * flags; a vertex outside [1, 2^28); first_index + n > 2^32 with indices NULL;
 * n >= 2^32; a null rays or out with n > 0; in the host variant a bad ray,
 * named in rt_last_error as rt_world_hit names it, or a non-finite or zero
 * eval direction, named by its index.  RT_EHANDLE / RT_EMOVED /
 * RT_EUNSUPPORTED / RT_ESTACK as rt_render gives them.  RT_EDEVICE without a
 * gfx950 device (there is no CPU fallback).  n == 0 is RT_OK, touches no
 * device and needs no arrays.  Host arrays, on the calling thread's current
 * device, blocking: */
int32_t rt_world_scatter(rt_scene* s, int32_t world, int32_t lights, const rt_scatter_opts* opts, const rt_ray* rays,
                         const double* eval_dirs3, const uint32_t* indices, uint64_t n, rt_scatter* out);
/* The same from and to gfx950 device arrays, enqueued on opts->stream without
 * waiting.  The arrays are the caller's duty, as in rt_world_hit_device; the
 * kernel ends and writes a record for any ray, and none past out_device[n - 1].
 * out_device must be 16-B aligned (RT_EINVAL otherwise): a record is written
 * as fourteen 16-B stores. */
int32_t rt_world_scatter_device(rt_scene* s, int32_t world, int32_t lights, const rt_scatter_opts* opts,
                                const rt_ray* rays_device, const double* eval_dirs3_device,
                                const uint32_t* indices_device, uint64_t n, rt_scatter* out_device);

/* Number of rows a shard renders (rows of the compact output). */
uint32_t rt_shard_rows(const rt_camera* cam, const rt_render_opts* opts);

/* Device-resident variant: out_linear_rgb_device is a gfx950 device pointer
 * (rows x W x 3 f32; on devices[0] when n_devices > 1; may be NULL on comm
 * ranks other than 0).  Enqueued on opts->stream and returns without waiting;
 * stats (if given) are filled by rt_render_device_wait.  Renders on one scene
 * are ordered: a call's device work starts after the previous call's on the
 * same device has finished (its stream waits on that call's completion
 * event), because they share the scene's per-device work buffers. */
int32_t rt_render_device(rt_scene* s, int32_t world, int32_t lights, const rt_camera* cam,
                         const rt_render_opts* opts, float* out_linear_rgb_device);
/* Waits for the last rt_render_device on this scene and reports its stats
 * (an earlier call's stats are superseded by a later call's). */
int32_t rt_render_device_wait(rt_scene* s, rt_stats* stats);
/* How the last render on this scene brought its parts to devices[0] / rank 0
 * (the transfer rt_stats.gather_ms times; the replacement of rayon's join of
 * the pixel iterator, camera.rs:178-197): RT_GATHER_NONE (one part, nothing
 * gathered), RT_GATHER_RCCL_COMM (one ncclSend / ncclRecv group over an
 * rt_comm_init communicator), RT_GATHER_RCCL_DEVICES (one group over the
 * ncclCommInitAll communicators of a device list), RT_GATHER_PEER_COPY
 * (hipMemcpyPeerAsync: a device listed twice, or librccl absent); < 0 when
 * nothing was rendered on the scene. */
#define RT_GATHER_NONE 0
#define RT_GATHER_RCCL_COMM 1
#define RT_GATHER_RCCL_DEVICES 2
#define RT_GATHER_PEER_COPY 3
int32_t rt_render_gather_mode(const rt_scene* s);

/* Test hook (parity tooling, not part of the reference surface): the f64 sum
 * of each (pixel, stratum row s_i) of the last single-device render on this
 * scene -- Sum over s_j of ray_color (camera.rs:183-192) before the 1/spp
 * scale -- laid out [rows x W][sqrt_spp][3].  n_values must equal
 * rows * W * sqrt_spp * 3.  Waits for the render. */
int32_t rt_render_partials_get(rt_scene* s, double* out, uint64_t n_values);

/* Test hook (parity tooling, not part of the reference surface): the
 * primary-ray candidate table of the last single-device render on this scene,
 * 8 sphere indices per pixel laid out [rows x W][8] -- ascending, 0xfffe in
 * the unused slots, 0xffff in slot 0 of a pixel whose primary rays walk the
 * tree.  n_values must equal rows * W * 8.  RT_EUNSUPPORTED when the render's
 * kernel builds no table (every tier but the basic one, and its wide
 * variant).  Waits for the render. */
int32_t rt_render_primary_get(rt_scene* s, uint16_t* out, uint64_t n_values);

/* Test hook (parity tooling, not part of the reference surface): n calls of
 * one f64 function on the current gfx950 device, from host arrays a (and b)
 * into out.  fn: 0 sin, 1 cos, 2 sincos's sin, 3 sincos's cos, 4 log (ln),
 * 5 acos, 6 atan2(a, b), 7 sqrt, 8 / 9 sin / cos of 2 pi a (a a unit draw,
 * the path's sincos_2pi), 10 0.0625^a for a in [0, 1] (rtcr::pow_2m4, the
 * clearcoat sampler's powf; impl 1: ocml's pow).  impl 0: the functions the render kernel
 * calls (rt_crmath.h: correctly rounded, in place of Rust's f64::sin / cos /
 * ln / acos / atan2 = glibc's); impl 1: ROCm's device libm (ocml).  Blocking. */
int32_t rt_math_selftest(int32_t fn, int32_t impl, const double* a, const double* b, double* out, uint64_t n);

/* Test hook (parity tooling, not part of the reference surface): n cases of
 * one f32 stage of the closest-hit walk on the current gfx950 device -- the
 * device functions the path kernels call -- from the host array `in` into
 * `out`, a fixed number of doubles per case; f32 quantities travel as doubles
 * that hold an f32 exactly.  fn (doubles in -> doubles out):
 *   0  box test: o[3], d[3], lo[3], hi[3], tmin_f, c_f -> hit (0 / 1), entry
 *   1  sphere filter: o[3], d[3], cx, cy, cz, r, g, c_f -> keep (0 / 1), c_f'
 *   2  the f32 reciprocal of the ray set-up: x -> r
 *   3  the f32 square root of the sphere filter's set-up: x -> r
 *   4  the closest hit's f32 bound set from t: t -> c_f
 *   5  that bound lowered by a hit t from c_f: t, c_f -> c_f'
 *   6  the largest f32 <= x: x -> r
 * Blocking. */
int32_t rt_walk_selftest(int32_t fn, const double* in, double* out, uint64_t n);

/* Test hook (parity tooling, not part of the reference surface): n cases of
 * the Disney BSDF's device functions as the path kernel's tier 5 compiles
 * them, on the current gfx950 device, for one parameter set and base colour;
 * host arrays, a fixed number of doubles per case.  fn:
 *   0  Disney::evaluate_disney (disney.rs:289-401): v_out[3], v_in[3] (both in
 *      the shading frame, y = the normal), front_face (0 / 1) ->
 *      reflectance[3], forward pdf, reverse pdf, panic (0 / 1)
 *   1  Disney::scatter's v_out, DisneyPDF::new and generate (disney.rs:77,
 *      524-540, 672-690) with the draws given instead of drawn: world
 *      normal[3], world -r_in.direction[3], front_face, four unit draws in call
 *      order -> 1 / 0 (Some / None), direction[3], draws consumed, panic
 * A case that panics (a reference unwrap / expect / assert!) is zeros and the
 * flag.  RT_EUNSUPPORTED in a build without the kernels.  Blocking. */
int32_t rt_disney_selftest(int32_t fn, const rt_disney_params* params, const double base_color[3], const double* in,
                           double* out, uint64_t n);

/* Test hook (host only, not part of the reference surface): builds
 * BVH::from_vec (bvh.rs:16-46) over the children of `list` twice, on copies
 * of the scene -- the parallel builder rt_bvh_new uses and the plain serial
 * recursion -- and returns 1 when the two give the same nodes (ids, children,
 * boxes bit for bit), 0 when they differ, < 0 on a bad argument.  The scene
 * is not modified. */
int32_t rt_bvh_selftest(rt_scene* s, int32_t list);
/* Test hook (host only): flattens (world, lights, background) for rt_render
 * twice -- the binned-SAH rebuild with both halves of large nodes built at
 * once, and serially -- and returns 1 when the flattened worlds agree (nodes,
 * lists, primitives, roots, stack need: bit for bit), 0 when not, < 0 on an
 * error.  The scene is not modified. */
int32_t rt_world_selftest(rt_scene* s, int32_t world, int32_t lights, int32_t background_tex);

/* ---- Multi-process communicator (RCCL) -------------------------------------- */
#define RT_COMM_ID_BYTES 128
/* ncclGetUniqueId: call on rank 0 and hand the bytes to every rank. */
int32_t rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
/* ncclCommInitRank on the calling thread's current HIP device; NULL on failure
 * (rt_last_error). */
rt_comm* rt_comm_init(const uint8_t id[RT_COMM_ID_BYTES], int32_t nranks, int32_t rank);
void rt_comm_destroy(rt_comm* comm);

/* ---- Output stage ---------------------------------------------------------- */
/* Color::to_rgb (utils/color.rs:27-36) of a device-resident linear framebuffer
 * (n_values f32 -> u8, toon_map 0 = None, 1 = ACES), enqueued on `stream`.
 * rt_render's out_srgb is the same conversion made from the f64 pixel sums. */
int32_t rt_to_rgb_device(const float* linear_device, uint8_t* srgb_device, uint64_t n_values, int32_t toon_map,
                         void* stream);
/* img.save(path) with std::fs::create_dir_all of its parent (main.rs:39-47):
 * 8-bit RGB PNG, row-major, y down. */
int32_t rt_write_png(const char* path, uint32_t width, uint32_t height, const uint8_t* rgb);
/* Camera::from_json (camera.rs:119-159) with the path given directly (the
 * reference looks in RTW_IMAGES, then ./assets): the CameraParams fields
 * (camera.rs:33-43) over rt_camera_default; a missing field or a malformed
 * file is RT_EINVAL (the reference's Err). */
int32_t rt_camera_from_json(const char* path, rt_camera* cam);

#ifdef __cplusplus
}
#endif
#endif /* RT_MI355X_H */
