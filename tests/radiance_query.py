"""Shared by tests/test_world_radiance_cpu.py and tests/test_world_radiance_gpu.py:
the oracle's radiance-query driver (tests/cpp/radiance_oracle.cpp, built once
per process and flavour as tests/disney_query.py builds its driver), one world
per kernel tier, and each world's ray set.

A world is `build(rt, scene, tmp) -> (world, lights, cam, box)`: `cam` gives
the camera-like half of the rays its origin and aim (and the background), `box`
= (lo, hi) is where the other half's origins are drawn.  WORLDS maps a name to
(build, kernel tier, lit): `lit` worlds hold an emitter the rays can end on.

RAYS rays a world, fixed by RAY_SEED: half from the camera's position towards
a plane 1.3 times its field of view wide (so some pass the objects by), half
from uniform points of `box` in uniform directions; every direction scaled to
a log-uniform length in [1e-3, 1e3]; a uniform time in [0, 1); t_max = +inf
but for every tenth ray, which takes a finite one from the oracle's first hit:
0.6 t (the hit lies beyond it: a miss), 1.7 t (it does not), in turn, and 10
for a ray that hits nothing.
"""
import ctypes as C
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT, pkg_module
import disney_query as dq
import hit_query as hq
import material_worlds as mw
import portal_query as pq
from test_lights_textures_gpu import _room

RAYS = 2048
RAY_SEED = 20251021   # numpy's, for the ray sets
SEED = 77             # the RNG contract's key of every query here
DEPTH = 8
_DP = C.POINTER(C.c_double)


# ---------------------------------------------------------------- the driver
@functools.lru_cache(maxsize=None)
def driver(crmath=True):
    """capi.Api of the oracle with the Disney and Portal materials, and
    orcx_world_radiance / orcx_camera_rays / orcx_first_hit bound as
    .x_world_radiance / .x_camera_rays / .x_first_hit (-DORC_CRMATH as
    liboracle_cr.so is built, or without it: glibc's libm)."""
    capi = pkg_module("capi")
    out = os.path.join(tempfile.mkdtemp(prefix="radiance_query_"), "libradiance_oracle%s.so" % ("_cr" if crmath else ""))
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off"] + (["-DORC_CRMATH"] if crmath else []) + \
          ["-shared", "-o", out, os.path.join(ROOT, "tests", "cpp", "radiance_oracle.cpp"),
           os.path.join(ROOT, "oracle", "rt_oracle.cpp"), os.path.join(ROOT, "oracle", "rt_oracle_obj.cpp"),
           "-pthread", "-lz"]
    subprocess.run(cmd, check=True, timeout=600)
    lib = C.CDLL(out)
    api = capi.Api(lib, "orc_", capi.ORACLE_EXTRAS)
    for name in ("orc_mat_portal", "orc_mat_disney", "orc_disney_params_default"):
        assert name not in api.missing, name
    fn = lib.orcx_world_radiance
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, _DP,
                   C.c_uint64, _DP]
    api.x_world_radiance = fn
    fn = lib.orcx_camera_rays
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.POINTER(capi.RtCamera), C.c_uint64, _DP, C.c_uint64]
    api.x_camera_rays = fn
    fn = lib.orcx_first_hit
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, _DP, C.c_uint64, _DP]
    api.x_first_hit = fn
    return api


def oracle_radiance(api, scene, world, lights, rays, *, max_depth=DEPTH, samples=1, seed=SEED, background=None,
                    first_index=0):
    """orcx_world_radiance for an (n, 8) ray array, as Scene.radiance returns
    it: (rgb (n, 3) f64, rays (n,) u32, panics (n,) u32)."""
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    raw = np.zeros((a.shape[0], 5), dtype=np.float64)
    api.check(api.x_world_radiance(scene.s, world.h, -1 if lights is None else lights.h,
                                   -1 if background is None else background.h, int(max_depth), int(samples), int(seed),
                                   int(first_index), a.ctypes.data_as(_DP), a.shape[0], raw.ctypes.data_as(_DP)))
    return raw[:, 0:3].copy(), raw[:, 3].astype(np.uint32), raw[:, 4].astype(np.uint32)


def camera_rays(api, scene, cam, seed):
    """orcx_camera_rays: cam.get_ray(i, j, 0, 0) of every pixel, (W * H, 8), row-major."""
    c = cam.to_c()
    n = cam.image_width * cam.image_height
    rays = np.zeros((n, 8), dtype=np.float64)
    api.check(api.x_camera_rays(scene.s, C.byref(c), int(seed), rays.ctypes.data_as(_DP), n))
    return rays


def first_hit(api, scene, world, rays, seed=SEED, first_index=0):
    """t of each ray's first world.hit over [1e-8, inf) on the oracle (sample 0's), -1 for a miss."""
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    t = np.zeros(a.shape[0], dtype=np.float64)
    api.check(api.x_first_hit(scene.s, world.h, int(seed), int(first_index), a.ctypes.data_as(_DP), a.shape[0],
                              t.ctypes.data_as(_DP)))
    return t


# ---------------------------------------------------------------- worlds
ROOM = ((5.0, 5.0, 5.0), (550.0, 550.0, 550.0))


def world_spheres(rt, s, tmp):
    """The random-spheres world of the 64 x 36 camera (basic tier, sky gradient)."""
    world, lights, cam = pkg_module("scenes").random_spheres(s, image_width=64, samples_per_pixel=1)
    return world, lights, cam, ((-11.0, 0.05, -11.0), (11.0, 3.0, 11.0))


def world_mc_obj(rt, s, tmp):
    """tests/golden/ref_assets/mc.obj as tests/hit_query.py loads it (vanilla
    metals under RemappedMaterials: the mesh tier), under a sky gradient."""
    world, cam, _ = hq.world_mc_obj(rt, s, tmp)
    cam.background = s.SkyGradient()
    # the ore cube and the pickaxe fill a narrow cone from the camera's position, and the box round them is tight
    cam.aspect_ratio, cam.vertical_fov_in_degrees = 1.0, 16.0
    return world, None, cam, ((-6.6, -6.9, -11.4), (-4.6, -4.9, -9.0))


def _material_world(name):
    def build(rt, s, tmp):
        world, lights, cam = mw.build(rt, s, name)
        return world, lights, cam, ROOM
    return build


def world_media(rt, s, tmp):
    """tests/test_flat_media_gpu.py's "spheres" room: a bare sphere of fog and
    one under a scaling, rotating Transform, lit by the ceiling quad (flat tier)."""
    world, cam = _room(s, rt, width=64, spp=16, depth=DEPTH)
    world.add(s.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), s.DiffuseLight(s.SolidColor((15.0, 15.0, 15.0)))))
    lights = s.Hittables()
    lights.add(s.Quad((343, 554, 332), (-130, 0, 0), (0, 0, -105), s.EmptyMaterial()))
    q2 = rt.Quaternion.from_axis_angle(s.api, (1, 0, 0), 10.0)
    world.add(s.ConstantMedium(s.Sphere((170, 120, 200), 110, s.EmptyMaterial()), 0.02, s.SolidColor((0.9, 0.9, 0.9))))
    world.add(s.ConstantMedium(s.Transform(s.Sphere((0, 0, 0), 80, s.EmptyMaterial()), (380, 150, 300), q2,
                                           (1.3, 0.8, 1.0)), 0.03, s.SolidColor((0.8, 0.2, 0.2))))
    return world, lights, cam, ROOM


def world_disney(rt, s, tmp):
    world, lights, cam = dq.WORLDS["lobes_lit"](s)
    return world, lights, cam, ROOM


def world_portal(rt, s, tmp):
    world, lights, cam = pq.WORLDS["wrapped"](s)
    return world, lights, cam, ((-5.0, 0.05, -2.0), (5.0, 3.6, 3.0))


# name -> (build, kernel tier, lit)
WORLDS = {
    "spheres": (world_spheres, 0, False),
    "mc_obj": (world_mc_obj, 1, False),
    "plain_bvh_lit": (_material_world("plain_bvh_lit"), 2, True),
    "uvwrap_flat_lit": (_material_world("uvwrap_flat_lit"), 3, True),
    "general_bvh_lit": (_material_world("general_bvh_lit"), 4, True),
    "noise_general": (_material_world("noise_general"), 4, True),
    "media": (world_media, 3, True),
    "disney": (world_disney, 5, True),
    "portal": (world_portal, 5, False),
}
# the worlds whose batches also run at every size of SIZES (tiers 0 and 2)
SIZED = ("spheres", "plain_bvh_lit")
SIZES = (1, 63, 64, 65, 257, 1023, 1025, 2048)


def world_case(api, name, tmp=None):
    """(scene, world, lights, cam, box) of a named world on `api`."""
    rt = pkg_module("raytracer")
    s = rt.Scene(api)
    world, lights, cam, box = WORLDS[name][0](rt, s, tmp or tempfile.mkdtemp(prefix="radiance_world_"))
    return s, world, lights, cam, box


# ---------------------------------------------------------------- rays
def _unit(v):
    return v / np.linalg.norm(v)


def ray_set(name, cam, box, hit):
    """The world's RAYS rays, (RAYS, 8); `hit(rays)` is the oracle's first-hit
    query (the finite t_max values are taken from it)."""
    g = np.random.default_rng(RAY_SEED + sorted(WORLDS).index(name))
    n_cam = RAYS // 2
    lf, la, up = (np.array(v, dtype=np.float64) for v in (cam.look_from, cam.look_at, cam.vec_up))
    w = _unit(lf - la)
    u = _unit(np.cross(up, w))
    v = np.cross(w, u)
    half_h = 1.3 * math.tan(math.radians(cam.vertical_fov_in_degrees) / 2.0)
    half_w = half_h * float(cam.aspect_ratio)
    a, b = g.uniform(-half_w, half_w, n_cam), g.uniform(-half_h, half_h, n_cam)
    rays = np.zeros((RAYS, 8))
    rays[:n_cam, 0:3] = lf
    rays[:n_cam, 3:6] = -w + a[:, None] * u + b[:, None] * v
    lo, hi = (np.array(x, dtype=np.float64) for x in box)
    rays[n_cam:, 0:3] = g.uniform(lo, hi, (RAYS - n_cam, 3))
    d = g.standard_normal((RAYS - n_cam, 3))
    rays[n_cam:, 3:6] = d
    length = 10.0 ** g.uniform(-3.0, 3.0, RAYS)
    rays[:, 3:6] *= (length / np.linalg.norm(rays[:, 3:6], axis=1))[:, None]
    rays[:, 6] = g.random(RAYS)
    rays[:, 7] = np.inf
    t = hit(rays)
    cut = np.arange(RAYS)[g.permutation(RAYS)[:RAYS // 10]]
    cut.sort()
    for k, i in enumerate(cut):
        rays[i, 7] = 10.0 if t[i] < 0 else t[i] * (0.6 if k % 2 == 0 else 1.7)
    return np.ascontiguousarray(rays)


@functools.lru_cache(maxsize=None)
def _oracle_world(name, crmath):
    return world_case(driver(crmath), name)


@functools.lru_cache(maxsize=None)
def world_rays(name):
    """(rays, first-hit t of sample 0) of a named world, made once per process
    on the ORC_CRMATH driver."""
    drv = driver(True)
    s, world, lights, cam, box = _oracle_world(name, True)
    rays = ray_set(name, cam, box, lambda r: first_hit(drv, s, world, r))
    t = first_hit(drv, s, world, rays)
    rays.setflags(write=False)
    t.setflags(write=False)
    return rays, t


@functools.lru_cache(maxsize=None)
def reference(name, samples=1, max_depth=DEPTH, crmath=True):
    """The driver's (rgb, rays, panics) for a named world's ray set, made once
    per process and left unchanged."""
    rays, _ = world_rays(name)
    s, world, lights, cam, _ = _oracle_world(name, crmath)
    out = oracle_radiance(driver(crmath), s, world, lights, rays, max_depth=max_depth, samples=samples,
                          background=cam.background)
    for a in out:
        a.setflags(write=False)
    return out


def within(g, o, rel=1e-5):
    """Per ray: every channel within rel * max(1, |oracle|)."""
    return np.all(np.abs(g - o) <= rel * np.maximum(1.0, np.abs(o)), axis=1)
