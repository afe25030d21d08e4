"""Host-side mirror of the reference's scene API over the C ABI.

Names and argument meanings follow the Rust crate `raytracer`
(/root/reference/src): textures (texture.rs), materials (material.rs), shapes
(shapes/*.rs, bvh.rs, hits.rs, volume.rs), Quaternion (utils/quaternion.rs)
and Camera (camera.rs).  A `Scene` is one `rt_scene` on one implementation of
the ABI; the gfx950 library is the product, and tests may hand the same scene
script the test-only oracle to compare against.

    scene = Scene(api)
    ground = scene.Lambertian(scene.SolidColor((0.5, 0.5, 0.5)))
    world = scene.Hittables()
    world.add(scene.Sphere((0, -1000, 0), 1000, ground))
    cam = Camera(); cam.image_width = 400; ...
    img = cam.render(world, None)          # Camera::render, camera.rs:161
"""
import ctypes as C
import math
import os

import numpy as np

from .capi import (OBJ_DISNEY, OBJ_VANILLA, Api, RtCamera, RtDisneyParams, RtError, RtHitRecord, RtLightSample,
                   RtLightsOpts, RtRadiance, RtRadianceOpts, RtRay, RtRenderOpts, RtScatter, RtScatterOpts, RtStats, d3,
                   d4)

# rt_hit_record as a numpy record (80 B, the C layout)
HIT_DTYPE = np.dtype([("t", "<f8"), ("p", "<f8", (3,)), ("normal", "<f8", (3,)), ("u", "<f8"), ("v", "<f8"),
                      ("mat", "<i4"), ("flags", "<u4")])
assert HIT_DTYPE.itemsize == C.sizeof(RtHitRecord)
# rt_radiance as a numpy record (32 B, the C layout)
RADIANCE_DTYPE = np.dtype([("rgb", "<f8", (3,)), ("rays", "<u4"), ("panics", "<u4")])
assert RADIANCE_DTYPE.itemsize == C.sizeof(RtRadiance)
# rt_light_sample as a numpy record (40 B, the C layout)
LIGHT_SAMPLE_DTYPE = np.dtype([("dir", "<f8", (3,)), ("pdf", "<f8"), ("flags", "<u4"), ("reserved", "<u4")])
assert LIGHT_SAMPLE_DTYPE.itemsize == C.sizeof(RtLightSample)
# rt_scatter as a numpy record (224 B, the C layout)
SCATTER_DTYPE = np.dtype([("hit", HIT_DTYPE), ("emitted", "<f8", (3,)), ("f", "<f8", (3,)), ("pdf", "<f8"),
                          ("origin", "<f8", (3,)), ("dir", "<f8", (3,)), ("eval_f", "<f8", (3,)), ("eval_pdf", "<f8"),
                          ("flags", "<u4"), ("draws", "<u4")])
assert SCATTER_DTYPE.itemsize == C.sizeof(RtScatter)


class Texture:
    def __init__(self, scene, h):
        self.scene, self.h = scene, h


class Material:
    def __init__(self, scene, h):
        self.scene, self.h = scene, h


class Hittable:
    """An owned object handle (Box<dyn Hittable>)."""

    def __init__(self, scene, h, kind):
        self.scene, self.h, self.kind = scene, h, kind


class Hittables(Hittable):
    """hits.rs:9-76 -- `add` moves the object in (hits.rs:27-30)."""

    def add(self, obj):
        self.scene.api.check(self.scene.api.hittables_add(self.scene.s, self.h, obj.h))


class Quaternion:
    """utils/quaternion.rs -- (w, x, y, z); constructors evaluated by the library."""

    def __init__(self, w=1.0, x=0.0, y=0.0, z=0.0):
        self.wxyz = (float(w), float(x), float(y), float(z))

    @staticmethod
    def identity():
        return Quaternion()

    @staticmethod
    def from_axis_angle(api, axis, angle_in_degrees):
        out = (C.c_double * 4)()
        api.check(api.quat_from_axis_angle(d3(axis), float(angle_in_degrees), out))
        return Quaternion(*out)

    @staticmethod
    def from_euler(api, yaw, pitch, roll):
        out = (C.c_double * 4)()
        api.quat_from_euler(float(yaw), float(pitch), float(roll), out)
        return Quaternion(*out)


class Scene:
    def __init__(self, api: Api):
        self.api = api
        self.s = api.scene_create()
        if not self.s:
            raise RtError(-8, "scene_create failed")

    def close(self):
        if self.s:
            self.api.scene_destroy(self.s)
            self.s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _c(self, rc):
        return self.api.check(rc)

    # ---- textures (texture.rs)
    def SolidColor(self, rgb):
        return Texture(self, self._c(self.api.tex_solid(self.s, d3(rgb))))

    def CheckerTexture(self, scale, even, odd):
        return Texture(self, self._c(self.api.tex_checker(self.s, float(scale), even.h, odd.h)))

    def ImageTexture(self, rgba=None, linear_interp=False):
        """rgba: HxWx4 float32 linear, or None for a missing file (cyan)."""
        if rgba is None:
            return Texture(self, self._c(self.api.tex_image(self.s, 0, 0, None, int(linear_interp))))
        a = np.ascontiguousarray(rgba, dtype=np.float32)
        h, w = a.shape[:2]
        ptr = a.ctypes.data_as(C.POINTER(C.c_float))
        return Texture(self, self._c(self.api.tex_image(self.s, w, h, ptr, int(linear_interp))))

    def ImageTexture_file(self, path, raw=False, linear_interp=None):
        """ImageTexture::new(file) / new_raw_image(file) (texture.rs:82-97) with
        the path given directly; PNG, JPEG and Radiance HDR decoded by the
        library, the format taken from the extension (missing -> cyan)."""
        interp = raw if linear_interp is None else linear_interp
        return Texture(self, self._c(self.api.tex_image_file(self.s, os.fsencode(path), int(raw), int(interp))))

    def NoiseTexture(self, scale, seed=0):
        return Texture(self, self._c(self.api.tex_noise(self.s, float(scale), int(seed))))

    def SkyGradient(self, horizon=(1.0, 1.0, 1.0), zenith=(0.5, 0.7, 1.0)):
        return Texture(self, self._c(self.api.tex_sky_gradient(self.s, d3(horizon), d3(zenith))))

    # ---- materials (material.rs)
    def EmptyMaterial(self):
        return Material(self, self._c(self.api.mat_empty(self.s)))

    def Lambertian(self, tex):
        return Material(self, self._c(self.api.mat_lambertian(self.s, tex.h)))

    def Metal(self, albedo, fuzz):
        return Material(self, self._c(self.api.mat_metal(self.s, d3(albedo), float(fuzz))))

    def Dielectric(self, tex, refraction_index):
        return Material(self, self._c(self.api.mat_dielectric(self.s, tex.h, float(refraction_index))))

    def DiffuseLight(self, tex, material=None):
        return Material(self, self._c(self.api.mat_diffuse_light(self.s, tex.h, -1 if material is None else material.h)))

    def Isotropic(self, tex):
        return Material(self, self._c(self.api.mat_isotropic(self.s, tex.h)))

    def Transparent(self):
        return Material(self, self._c(self.api.mat_transparent(self.s)))

    def Mix(self, mat1, mat2, ratio):
        return Material(self, self._c(self.api.mat_mix(self.s, mat1.h, mat2.h, float(ratio))))

    def Mix_from_image(self, mat1, mat2, image_tex):
        """Mix::from_image (material.rs:235-247): ratio = the texture's alpha."""
        return Material(self, self._c(self.api.mat_mix_image(self.s, mat1.h, mat2.h, image_tex.h)))

    def disney_params(self, **params):
        """rt_disney_params: DisneyParameters::default (disney.rs:36-55) with the given fields set."""
        p = RtDisneyParams()
        self.api.disney_params_default(C.byref(p))
        for name, value in params.items():
            if name in ("struct_size",) or not hasattr(p, name):
                raise TypeError(f"unknown Disney parameter {name!r}")
            setattr(p, name, int(bool(value)) if name == "thin" else float(value))
        return p

    def Disney(self, tex, **params):
        """Disney::builder()...build() with base_color from `tex` at the hit
        (material/disney.rs:59-61, obj.rs:279-292); `params`: roughness,
        anisotropic, sheen, sheen_tint, clearcoat, clearcoat_gloss,
        specular_tint, metallic, ior, flatness, spec_trans, diff_trans, thin."""
        p = self.disney_params(**params)
        return Material(self, self._c(self.api.mat_disney(self.s, tex.h, C.byref(p))))

    def Portal(self, attenuation, offset=None, rotation=None):
        """Portal::new(attenuation, position_offset, rotation)
        (material/portal.rs:15-25): the ray goes on from rec.p + offset along
        rotation.rotate_vector(direction), tinted by `attenuation`.  `rotation`
        is a Quaternion, used as given (not normalised); None = identity,
        offset None = zero."""
        off = d3(offset) if offset is not None else None
        q = d4(rotation.wxyz) if rotation is not None else None
        return Material(self, self._c(self.api.mat_portal(self.s, d3(attenuation), off, q)))

    # ---- hittables
    def Sphere(self, center, radius, mat):
        return Hittable(self, self._c(self.api.sphere(self.s, d3(center), float(radius), mat.h)), "sphere")

    def Sphere_new_with_motion(self, center1, center2, radius, mat):
        return Hittable(self, self._c(self.api.sphere_moving(self.s, d3(center1), d3(center2), float(radius), mat.h)), "sphere")

    def Quad(self, anchor, u, v, mat):
        return Hittable(self, self._c(self.api.quad(self.s, d3(anchor), d3(u), d3(v), mat.h)), "quad")

    def Triangle(self, anchor, u, v, mat):
        """Triangle::new -> Option: None when degenerate (triangle.rs:29-31)."""
        rc = self.api.triangle(self.s, d3(anchor), d3(u), d3(v), mat.h)
        if rc == -4:
            return None
        return Hittable(self, self._c(rc), "triangle")

    def Hittables(self):
        return Hittables(self, self._c(self.api.hittables_new(self.s)), "list")

    def BVH(self, hittables):
        return Hittable(self, self._c(self.api.bvh_new(self.s, hittables.h)), "bvh")

    def build_box(self, a, b, mat):
        return Hittables(self, self._c(self.api.build_box(self.s, d3(a), d3(b), mat.h)), "list")

    def Transform(self, obj, offset=None, quaternion=None, scale=None):
        off = d3(offset) if offset is not None else None
        q = d4(quaternion.wxyz) if quaternion is not None else None
        sc = d3(scale) if scale is not None else None
        return Hittable(self, self._c(self.api.transform_new(self.s, obj.h, off, q, sc)), "transform")

    def ConstantMedium(self, boundary, density, tex):
        return Hittable(self, self._c(self.api.constant_medium_new(self.s, boundary.h, float(density), tex.h)), "medium")

    def Wavefont(self, obj_path, vanilla_material=True, disney=False):
        """Wavefont::new (shapes/obj.rs:117-134); returns the Hittables of its
        per-model BVHs.  The reference's Option<Wavefont> is None when the OBJ
        cannot be opened: here that raises RtError(RT_EINVAL).  disney=True is
        Wavefont::new in full (rt_wavefront_load_flags with RT_OBJ_DISNEY):
        every material that is no vanilla Metal / Dielectric becomes the Disney
        of obj.rs:279-292; with disney=False the old entry point is called and
        refuses such a material (RT_EUNSUPPORTED)."""
        path = os.fsencode(obj_path)
        if disney:
            rc = self.api.wavefront_load_flags(self.s, path, OBJ_DISNEY | (OBJ_VANILLA if vanilla_material else 0))
        else:
            rc = self.api.wavefront_load(self.s, path, 1 if vanilla_material else 0)
        return Hittables(self, self._c(rc), "list")

    # ---- Hittable::hit (hit.rs:46-60)
    def hit(self, world, rays, seed=0, flags=0):
        """world.hit(Ray{origin, dir, time}, [1e-8, t_max]) for each row
        (ox, oy, oz, dx, dy, dz, time, t_max) of the (n, 8) float64 array
        `rays` (rt_world_hit).  Returns n records as a numpy structured array
        (HIT_DTYPE: t, p, normal, u, v, mat, flags)."""
        a = np.ascontiguousarray(rays, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("rays must be an (n, 8) array: origin, direction, time, t_max")
        n = a.shape[0]
        out = np.zeros(n, dtype=HIT_DTYPE)
        self._c(self.api.world_hit(self.s, world.h, int(seed), int(flags), a.ctypes.data_as(C.POINTER(RtRay)), n,
                                   out.ctypes.data_as(C.POINTER(RtHitRecord))))
        return out

    def hit_device(self, world, rays_ptr, n, out_ptr, seed=0, flags=0, stream=None):
        """rt_world_hit_device: n rt_ray at the device address rays_ptr, n
        rt_hit_record written at out_ptr, enqueued on `stream` (a hipStream_t
        as an integer; None = the default stream) without waiting."""
        self._c(self.api.world_hit_device(self.s, world.h, int(seed), int(flags), C.c_void_p(int(rays_ptr)), int(n),
                                          C.c_void_p(int(out_ptr)), C.c_void_p(stream) if stream else None))

    # ---- Hittable::hit(..).is_some(): any-hit queries (shadow rays, visibility, ambient occlusion)
    def occluded(self, world, rays, seed=0, flags=0):
        """Whether world.hit(Ray{origin, dir, time}, [1e-8, t_max]) is Some for
        each row of the (n, 8) float64 array `rays`, as `hit` takes them
        (rt_world_occluded).  Returns an (n,) uint8 array of 0 / 1: the
        RT_HIT_FOUND bit of the record `hit` returns for that ray.  A segment
        test from a to b is the ray (a, b - a) with t_max just under 1."""
        a = np.ascontiguousarray(rays, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("rays must be an (n, 8) array: origin, direction, time, t_max")
        n = a.shape[0]
        out = np.zeros(n, dtype=np.uint8)
        self._c(self.api.world_occluded(self.s, world.h, int(seed), int(flags), a.ctypes.data_as(C.POINTER(RtRay)), n,
                                        out.ctypes.data_as(C.POINTER(C.c_uint8))))
        return out

    def occluded_device(self, world, rays_ptr, n, out_ptr, seed=0, flags=0, stream=None):
        """rt_world_occluded_device: n rt_ray at the device address rays_ptr, n
        bytes written at out_ptr, enqueued on `stream` (a hipStream_t as an
        integer; None = the default stream) without waiting."""
        self._c(self.api.world_occluded_device(self.s, world.h, int(seed), int(flags), C.c_void_p(int(rays_ptr)),
                                               int(n), C.c_void_p(int(out_ptr)),
                                               C.c_void_p(stream) if stream else None))

    # ---- Camera::ray_color (camera.rs:275-325) for caller-given rays
    def _radiance_opts(self, max_depth, samples, seed, background, first_index, flags, stream=None):
        o = RtRadianceOpts()
        self.api.radiance_opts_default(C.byref(o))
        o.max_depth, o.samples, o.seed = int(max_depth), int(samples), int(seed)
        o.background_tex = -1 if background is None else background.h
        o.first_index, o.flags = int(first_index), int(flags)
        o.stream = C.c_void_p(stream) if stream else None
        return o

    def radiance(self, world, lights, rays, *, max_depth=10, samples=1, seed=0, background=None, first_index=0, flags=0):
        """Camera::ray_color(Ray{origin, dir, time}, max_depth, world, lights)
        for each row of the (n, 8) float64 array `rays`, as `hit` takes them,
        `samples` times a ray (rt_world_radiance).  `background` is a Texture
        (Camera.background) or None for black; t_max bounds the first hit
        only; the RNG pixel of ray i is first_index + i.  Returns (rgb (n, 3)
        float64: the mean over the samples, rays (n,) uint32: ray_color calls,
        panics (n,) uint32: samples that panicked)."""
        a = np.ascontiguousarray(rays, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("rays must be an (n, 8) array: origin, direction, time, t_max")
        n = a.shape[0]
        out = np.zeros(n, dtype=RADIANCE_DTYPE)
        o = self._radiance_opts(max_depth, samples, seed, background, first_index, flags)
        self._c(self.api.world_radiance(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                        a.ctypes.data_as(C.POINTER(RtRay)), n, out.ctypes.data_as(C.POINTER(RtRadiance))))
        return out["rgb"].copy(), out["rays"].copy(), out["panics"].copy()

    def radiance_device(self, world, lights, rays_ptr, n, out_ptr, *, max_depth=10, samples=1, seed=0, background=None,
                        first_index=0, flags=0, stream=None):
        """rt_world_radiance_device: n rt_ray at the device address rays_ptr, n
        rt_radiance (RADIANCE_DTYPE) written at out_ptr, enqueued on `stream`
        (a hipStream_t as an integer; None = the default stream) without
        waiting."""
        o = self._radiance_opts(max_depth, samples, seed, background, first_index, flags, stream)
        self._c(self.api.world_radiance_device(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                               C.c_void_p(int(rays_ptr)), int(n), C.c_void_p(int(out_ptr))))

    # ---- one ray_color level: Material::emitted / ::scatter and the PDF (camera.rs:286-316)
    def _scatter_opts(self, seed, sample, vertex, first_index, background, flags, stream=None):
        o = RtScatterOpts()
        self.api.scatter_opts_default(C.byref(o))
        o.seed, o.sample, o.vertex, o.first_index, o.flags = int(seed), int(sample), int(vertex), int(first_index), int(flags)
        o.background_tex = -1 if background is None else background.h
        o.stream = C.c_void_p(stream) if stream else None
        return o

    def scatter(self, world, lights, rays, *, eval_dirs=None, indices=None, seed=0, sample=0, vertex=1, first_index=0,
                background=None, flags=0):
        """One ray_color level for each row of the (n, 8) float64 array `rays`,
        as `hit` takes them (rt_world_scatter): the hit record, what the
        surface emits, and Material::scatter -- a ray with its attenuation, or
        a PDF's generate() with its value -- without the lights mix.
        `eval_dirs` ((n, 3) float64 or None): directions whose PDF::value is
        returned too (eval_f, eval_pdf).  `indices` ((n,) uint32 or None): the
        RNG pixel of each ray, first_index + i when None; `sample` and `vertex`
        are the key's other coordinates.  `lights` only names the flattening.
        Returns n records as a numpy structured array (SCATTER_DTYPE)."""
        a = np.ascontiguousarray(rays, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 8:
            raise ValueError("rays must be an (n, 8) array: origin, direction, time, t_max")
        n = a.shape[0]
        e = i = None
        if eval_dirs is not None:
            e = self._triples(eval_dirs, "eval_dirs")
            if e.shape[0] != n:
                raise ValueError("eval_dirs must have one row a ray")
        if indices is not None:
            i = np.ascontiguousarray(indices, dtype=np.uint32)
            if i.shape != (n,):
                raise ValueError("indices must be an (n,) array")
        out = np.zeros(n, dtype=SCATTER_DTYPE)
        o = self._scatter_opts(seed, sample, vertex, first_index, background, flags)
        self._c(self.api.world_scatter(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                       a.ctypes.data_as(C.POINTER(RtRay)),
                                       e.ctypes.data_as(C.POINTER(C.c_double)) if e is not None else None,
                                       i.ctypes.data_as(C.POINTER(C.c_uint32)) if i is not None else None, n,
                                       out.ctypes.data_as(C.POINTER(RtScatter))))
        return out

    def scatter_device(self, world, lights, rays_ptr, n, out_ptr, *, eval_dirs_ptr=None, indices_ptr=None, seed=0,
                       sample=0, vertex=1, first_index=0, background=None, flags=0, stream=None):
        """rt_world_scatter_device: n rt_ray at the device address rays_ptr, n
        rt_scatter (SCATTER_DTYPE) written at the 16-B aligned out_ptr;
        eval_dirs_ptr (n packed triples of doubles) and indices_ptr (n uint32)
        are device addresses or None.  Enqueued on `stream` (a hipStream_t as
        an integer; None = the default stream) without waiting."""
        o = self._scatter_opts(seed, sample, vertex, first_index, background, flags, stream)
        self._c(self.api.world_scatter_device(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                              C.c_void_p(int(rays_ptr)),
                                              C.c_void_p(int(eval_dirs_ptr)) if eval_dirs_ptr else None,
                                              C.c_void_p(int(indices_ptr)) if indices_ptr else None, int(n),
                                              C.c_void_p(int(out_ptr))))

    # ---- Hittable::pdf_value / ::random of the lights (hit.rs:46-60, pdf.rs:66-88)
    def _lights_opts(self, samples=1, seed=0, first_index=0, background=None, flags=0, stream=None):
        o = RtLightsOpts()
        self.api.lights_opts_default(C.byref(o))
        o.samples, o.seed, o.first_index, o.flags = int(samples), int(seed), int(first_index), int(flags)
        o.background_tex = -1 if background is None else background.h
        o.stream = C.c_void_p(stream) if stream else None
        return o

    @staticmethod
    def _triples(a, name):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError(f"{name} must be an (n, 3) array")
        return a

    def lights_pdf(self, world, lights, origins, dirs, **opts):
        """lights.pdf_value(origin, dir) for each row of the (n, 3) float64
        arrays `origins` and `dirs` (rt_lights_pdf); the directions are used as
        given.  `world`, `background` (a Texture or None) and `flags` name the
        flattening, as for a render.  Returns an (n,) float64 array."""
        o_, d_ = self._triples(origins, "origins"), self._triples(dirs, "dirs")
        if o_.shape != d_.shape:
            raise ValueError("origins and dirs must have the same shape")
        n = o_.shape[0]
        out = np.zeros(n, dtype=np.float64)
        o = self._lights_opts(**opts)
        dp = C.POINTER(C.c_double)
        self._c(self.api.lights_pdf(self.s, world.h, -1 if lights is None else lights.h, C.byref(o), o_.ctypes.data_as(dp),
                                    d_.ctypes.data_as(dp), n, out.ctypes.data_as(dp)))
        return out

    def lights_sample(self, world, lights, origins, samples=1, seed=0, first_index=0, **opts):
        """`samples` draws of lights.random(origin) for each row of the (n, 3)
        float64 array `origins`, each with its lights.pdf_value
        (rt_lights_sample); the RNG pixel of origin i is first_index + i.
        Returns an (n, samples) array of LIGHT_SAMPLE_DTYPE: dir, pdf, flags
        (capi.LIGHT_PANIC: random panicked, dir and pdf are zero)."""
        o_ = self._triples(origins, "origins")
        n = o_.shape[0]
        out = np.zeros((n, max(int(samples), 0)), dtype=LIGHT_SAMPLE_DTYPE)
        o = self._lights_opts(samples, seed, first_index, **opts)
        self._c(self.api.lights_sample(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                       o_.ctypes.data_as(C.POINTER(C.c_double)), n,
                                       out.ctypes.data_as(C.POINTER(RtLightSample))))
        return out

    def lights_pdf_device(self, world, lights, origins_ptr, dirs_ptr, n, out_ptr, **opts):
        """rt_lights_pdf_device: n packed triples of doubles at each of the
        device addresses origins_ptr and dirs_ptr, n doubles written at out_ptr,
        enqueued on `stream` (a hipStream_t as an integer; None = the default
        stream) without waiting."""
        o = self._lights_opts(**opts)
        self._c(self.api.lights_pdf_device(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                           C.c_void_p(int(origins_ptr)), C.c_void_p(int(dirs_ptr)), int(n),
                                           C.c_void_p(int(out_ptr))))

    def lights_sample_device(self, world, lights, origins_ptr, n, out_ptr, samples=1, seed=0, first_index=0, **opts):
        """rt_lights_sample_device: n packed triples at origins_ptr, n * samples
        rt_light_sample (LIGHT_SAMPLE_DTYPE) written at out_ptr, likewise."""
        o = self._lights_opts(samples, seed, first_index, **opts)
        self._c(self.api.lights_sample_device(self.s, world.h, -1 if lights is None else lights.h, C.byref(o),
                                              C.c_void_p(int(origins_ptr)), int(n), C.c_void_p(int(out_ptr))))


class Camera:
    """camera.rs:45-104 -- pub fields with Camera::default values."""

    def __init__(self):
        self.aspect_ratio = 1.0
        self.image_width = 100
        self.samples_per_pixel = 10
        self.max_depth = 10
        self.background = None  # Texture; None = SolidColor(BLACK)
        self.vertical_fov_in_degrees = 90.0
        self.look_from = (0.0, 0.0, 0.0)
        self.look_at = (0.0, 0.0, -1.0)
        self.vec_up = (0.0, 1.0, 0.0)
        self.defocus_angle_in_degrees = 0.0
        self.focus_distance = 10.0
        self.toon_map = 0  # ToonMap::None

    @staticmethod
    def from_json(api, path):
        """Camera::from_json (camera.rs:119-159): the CameraParams fields from a
        JSON file over Camera::default (path given directly).  An
        implementation without rt_camera_from_json (a CPU one: file I/O is the
        product library's) gets the same fields through Python's json."""
        cam = Camera()
        if not hasattr(api, "camera_from_json"):
            import json
            with open(path, encoding="utf-8") as f:
                params = json.load(f)
            for name in ("aspect_ratio", "vertical_fov_in_degrees", "defocus_angle_in_degrees", "focus_distance"):
                setattr(cam, name, float(params[name]))
            cam.image_width = int(params["image_width"])
            for name in ("look_from", "look_at", "vec_up"):
                setattr(cam, name, tuple(float(x) for x in params[name]))
            return cam
        c = RtCamera()
        api.check(api.camera_from_json(os.fsencode(path), C.byref(c)))
        cam.aspect_ratio = c.aspect_ratio
        cam.image_width = c.image_width
        cam.vertical_fov_in_degrees = c.vertical_fov_in_degrees
        cam.look_from = tuple(c.look_from)
        cam.look_at = tuple(c.look_at)
        cam.vec_up = tuple(c.vec_up)
        cam.defocus_angle_in_degrees = c.defocus_angle_in_degrees
        cam.focus_distance = c.focus_distance
        return cam

    def to_c(self):
        c = RtCamera()
        c.aspect_ratio = float(self.aspect_ratio)
        c.image_width = int(self.image_width)
        c.samples_per_pixel = int(self.samples_per_pixel)
        c.max_depth = int(self.max_depth)
        c.background_tex = -1 if self.background is None else self.background.h
        c.vertical_fov_in_degrees = float(self.vertical_fov_in_degrees)
        c.look_from = d3(self.look_from)
        c.look_at = d3(self.look_at)
        c.vec_up = d3(self.vec_up)
        c.defocus_angle_in_degrees = float(self.defocus_angle_in_degrees)
        c.focus_distance = float(self.focus_distance)
        c.toon_map = int(self.toon_map)
        return c

    @property
    def image_height(self):
        h = int(self.image_width / self.aspect_ratio)
        return max(h, 1)

    @property
    def sqrt_spp(self):
        return int(math.sqrt(self.samples_per_pixel))

    def traced_samples(self):
        """pixels x floor(sqrt(spp))^2 -- what camera.rs:183-192 traces."""
        return self.image_width * self.image_height * self.sqrt_spp ** 2

    @staticmethod
    def _opts(api, seed, row_offset, row_stride, threads, flags, devices=None, comm=None):
        opts = RtRenderOpts()
        api.render_opts_default(C.byref(opts))
        opts.seed = int(seed)
        opts.row_offset = int(row_offset)
        opts.row_stride = int(row_stride)
        opts.threads = int(threads)
        opts.flags = int(flags)
        keep = None
        if devices is not None and len(devices) > 1:
            keep = (C.c_int32 * len(devices))(*[int(d) for d in devices])
            opts.n_devices = len(devices)
            opts.devices = C.cast(keep, C.POINTER(C.c_int32))
        if comm is not None:
            opts.comm = comm
        return opts, keep

    def render(self, world, lights=None, seed=1, row_offset=0, row_stride=1, threads=0, want_srgb=True, flags=0,
               devices=None, comm=None):
        """Camera::render (camera.rs:161).  Returns (linear HxWx3 f32, srgb HxWx3 u8 or None, RtStats).
        devices: HIP device ordinals to split the rows over (in-process
        multi-GPU, one gather onto devices[0]); comm: an rt_comm* of
        rt_comm_init (one process per GPU; the frame arrives on rank 0)."""
        scene = world.scene
        api = scene.api
        cam = self.to_c()
        opts, _keep = self._opts(api, seed, row_offset, row_stride, threads, flags, devices, comm)
        rows = api.shard_rows(C.byref(cam), C.byref(opts))
        W = self.image_width
        lin = np.zeros((rows, W, 3), dtype=np.float32)
        srgb = np.zeros((rows, W, 3), dtype=np.uint8) if want_srgb else None
        stats = RtStats()
        rc = api.render(scene.s, world.h, -1 if lights is None else lights.h, C.byref(cam), C.byref(opts),
                        lin.ctypes.data_as(C.POINTER(C.c_float)),
                        srgb.ctypes.data_as(C.POINTER(C.c_uint8)) if srgb is not None else None, C.byref(stats))
        api.check(rc)
        return lin, srgb, stats

    def render_partials(self, world, lights=None, seed=1, row_offset=0, row_stride=1, threads=0, flags=0):
        """Parity tooling: the f64 sum over s_j of ray_color for every (pixel,
        stratum row s_i) of the shard, (rows, W, sqrt_spp, 3) -- the GPU's
        per-item sums (rt_render_partials_get) or the oracle's
        (orc_render_partials).  Returns (partials, RtStats)."""
        scene = world.scene
        api = scene.api
        cam = self.to_c()
        opts, _keep = self._opts(api, seed, row_offset, row_stride, threads, flags)
        rows = api.shard_rows(C.byref(cam), C.byref(opts))
        S = self.sqrt_spp
        part = np.zeros((rows, self.image_width, S, 3), dtype=np.float64)
        stats = RtStats()
        lh = -1 if lights is None else lights.h
        ptr = part.ctypes.data_as(C.POINTER(C.c_double))
        if hasattr(api, "render_partials"):  # the oracle
            api.check(api.render_partials(scene.s, world.h, lh, C.byref(cam), C.byref(opts), ptr, C.byref(stats)))
        else:
            api.check(api.render(scene.s, world.h, lh, C.byref(cam), C.byref(opts), None, None, C.byref(stats)))
            if part.size:
                api.check(api.render_partials_get(scene.s, ptr, part.size))
        return part, stats


def save_png(api, path, srgb):
    """img.save(path) after create_dir_all (main.rs:39-47): srgb is HxWx3 u8."""
    a = np.ascontiguousarray(srgb, dtype=np.uint8)
    h, w = a.shape[:2]
    api.check(api.write_png(os.fsencode(path), w, h, a.ctypes.data_as(C.c_void_p)))
