"""Shared by tests/test_lights_query_cpu.py and tests/test_lights_query_gpu.py:
the oracle's lights-query driver (tests/cpp/lights_oracle.cpp, built once per
process as tests/hit_query.py builds its driver), six light sets -- the
issue's five and `deep`, which uses all four list / Transform levels a lights
tree may have -- and each set's origins and directions.

A light set is `build(rt, scene) -> (world, lights, cam)` through the rt.Scene
script, so that one builder drives the product and the oracle: the lights
object, beside a small world -- a floor quad, two spheres and a second copy of
the lights' shapes as emitters -- and a small camera for the tests that render.
Every leaf of a lights object has a DiffuseLight of its own (LEAVES[name] of
them, the scene's first materials), so orcx_world_hit on the lights object
names the leaf a direction meets first.

SETS maps a name to (box centre, box half-extent, the static sphere light
(centre, radius) origins are put into, or None, and the product of the list
sizes above that sphere: inside it pdf_value is at least 1 / 4 pi over that).

N origins a set, fixed by POINT_SEED: most uniform in the box, a few
light-sizes round the lights; where the set has a sphere light 64 inside it
(Sphere::pdf_value's NaN branch, 1 / 4 pi; Sphere::random panics there) and 1
exactly at its centre (random panics: the direction cannot be normalised); 8 at
1e3 and 8 at 1e-3 light-sizes from the box centre.  Directions of the pdf
query: every even index aims at a point the oracle's own Hittable::random drew
on the lights (where that draw panicked: isotropic), every odd index is
isotropic; every direction scaled to a log-uniform length in [1e-3, 1e3].
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

from conftest import ROOT, pkg_module

N = 4096
POINT_SEED = 20261021  # numpy's, for the point sets
AIM_SEED = 5           # the RNG contract's key of the draws the pdf directions aim at
SEED = 97              # ... and of every sample query here (the centre origin of `flat` and `tree`: some draws panic, some do not)
SAMPLES = 3
PANIC = 1
_DP = C.POINTER(C.c_double)


# ---------------------------------------------------------------- the driver
@functools.lru_cache(maxsize=None)
def driver():
    """capi.Api of the oracle (-DORC_CRMATH, as liboracle_cr.so is built) with
    orcx_lights_pdf / orcx_lights_sample / orcx_world_hit bound as
    .x_lights_pdf / .x_lights_sample / .x_world_hit."""
    capi = pkg_module("capi")
    out = os.path.join(tempfile.mkdtemp(prefix="lights_query_"), "liblights_oracle_cr.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DORC_CRMATH", "-shared", "-o", out,
           os.path.join(ROOT, "tests", "cpp", "lights_oracle.cpp"), os.path.join(ROOT, "oracle", "rt_oracle.cpp"),
           os.path.join(ROOT, "oracle", "rt_oracle_obj.cpp"), "-pthread", "-lz"]
    subprocess.run(cmd, check=True, timeout=600)
    lib = C.CDLL(out)
    api = capi.Api(lib, "orc_", capi.ORACLE_EXTRAS)
    fn = lib.orcx_lights_pdf
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, _DP, _DP, C.c_uint64, _DP]
    api.x_lights_pdf = fn
    fn = lib.orcx_lights_sample
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, _DP, C.c_uint64, _DP]
    api.x_lights_sample = fn
    fn = lib.orcx_world_hit
    fn.restype = C.c_int32
    fn.argtypes = [C.c_void_p, C.c_int32, C.c_uint64, _DP, C.c_uint64, _DP]
    api.x_world_hit = fn
    return api


def _triples(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[1] == 3
    return a


def oracle_pdf(api, scene, lights, origins, dirs):
    """orcx_lights_pdf, as Scene.lights_pdf returns it: (n,) f64."""
    o, d = _triples(origins), _triples(dirs)
    assert o.shape == d.shape
    out = np.zeros(len(o), dtype=np.float64)
    api.check(api.x_lights_pdf(scene.s, lights.h, o.ctypes.data_as(_DP), d.ctypes.data_as(_DP), len(o),
                               out.ctypes.data_as(_DP)))
    return out


def oracle_sample(api, scene, lights, origins, samples=1, seed=SEED, first_index=0):
    """orcx_lights_sample, as Scene.lights_sample returns it: (n, samples) of LIGHT_SAMPLE_DTYPE."""
    rt = pkg_module("raytracer")
    o = _triples(origins)
    raw = np.zeros((len(o), samples, 5), dtype=np.float64)
    api.check(api.x_lights_sample(scene.s, lights.h, int(seed), int(first_index), int(samples), o.ctypes.data_as(_DP),
                                  len(o), raw.ctypes.data_as(_DP)))
    out = np.zeros((len(o), samples), dtype=rt.LIGHT_SAMPLE_DTYPE)
    out["dir"], out["pdf"], out["flags"] = raw[..., 0:3], raw[..., 3], raw[..., 4].astype(np.uint32)
    return out


def oracle_leaf(api, scene, lights, origins, dirs):
    """The material handle of the leaf of `lights` each ray (origin, dir) meets
    first over [1e-8, inf) at time 0 (orcx_world_hit), -1 for a miss."""
    o, d = _triples(origins), _triples(dirs)
    rays = np.zeros((len(o), 8), dtype=np.float64)
    rays[:, 0:3], rays[:, 3:6], rays[:, 7] = o, d, np.inf
    raw = np.zeros((len(o), 12), dtype=np.float64)
    api.check(api.x_world_hit(scene.s, lights.h, 0, rays.ctypes.data_as(_DP), len(o), raw.ctypes.data_as(_DP)))
    found = raw[:, 10].astype(np.uint32) & 1
    return np.where(found != 0, raw[:, 9].astype(np.int64), -1)


def same_bits(a, b):
    """f64 arrays equal as bit patterns, a NaN on both sides counting as equal."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | nan))


def same_samples(a, b):
    return a.shape == b.shape and same_bits(a["dir"], b["dir"]) and same_bits(a["pdf"], b["pdf"]) and \
        np.array_equal(a["flags"], b["flags"]) and not a["reserved"].any() and not b["reserved"].any()


# ---------------------------------------------------------------- light sets
QUAD = ((-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0))  # one_quad: a unit quad, its axis x = z = 0
SPHERE = ((0.3, 2.0, -0.2), 0.7)                               # one_sphere
FLAT_SPHERE = ((-3.0, 2.0, 0.4), 0.5)
TREE_SPHERE = ((0.4, 2.6, -0.3), 0.45)


def _one_quad(rt, s, m):
    return s.Quad(*QUAD, m[0])


def _one_sphere(rt, s, m):
    return s.Sphere(*SPHERE, m[0])


def _one_triangle(rt, s, m):
    return s.Triangle((-0.6, 2.1, -0.4), (1.3, 0.1, 0.2), (0.2, -0.3, 1.1), m[0])


def _flat(rt, s, m):
    """A list of a sphere, a quad and a triangle (flattener light kind 1), far
    enough apart that from round the origin no direction meets two of them."""
    l = s.Hittables()
    l.add(s.Sphere(*FLAT_SPHERE, m[0]))
    l.add(s.Quad((-0.5, 3.0, -0.5), (1.0, 0.0, 0.1), (0.0, 0.2, 1.0), m[1]))
    l.add(s.Triangle((2.6, 1.8, -0.5), (0.9, 0.2, 0.0), (0.1, 0.4, 1.0), m[2]))
    return l


def _tree(rt, s, m):
    """Flattener light kind 2: a list of (a Transform -- non-uniform scale, a
    rotation about no axis of the frame, an offset -- over a list of a quad and
    a moving sphere), a plain sphere, and a list of a triangle and a Transform
    over a sphere."""
    inner = s.Hittables()
    inner.add(s.Quad((-0.4, 0.0, -0.3), (0.8, 0.0, 0.1), (0.0, 0.1, 0.7), m[0]))
    inner.add(s.Sphere_new_with_motion((0.9, 0.5, 0.2), (1.2, 0.7, 0.2), 0.3, m[1]))
    q = rt.Quaternion.from_axis_angle(s.api, (1.0, 2.0, -0.5), 37.0)
    l = s.Hittables()
    l.add(s.Transform(inner, (-2.5, 2.2, 0.5), q, (1.3, 0.7, 1.9)))
    l.add(s.Sphere(*TREE_SPHERE, m[2]))
    pair = s.Hittables()
    pair.add(s.Triangle((2.2, 1.6, -0.6), (0.9, 0.3, 0.1), (0.0, 0.5, 1.0), m[3]))
    q2 = rt.Quaternion.from_axis_angle(s.api, (0.3, 1.0, 0.2), 71.0)
    pair.add(s.Transform(s.Sphere((0.0, 0.0, 0.0), 0.4, m[4]), (2.4, 3.1, 1.2), q2, (1.0, 1.6, 0.8)))
    l.add(pair)
    return l


DEEP_SPHERE = ((-0.6, 2.9, 0.8), 0.4)


def _deep(rt, s, m):
    """Flattener light kind 2 at its depth limit, four list / Transform levels
    over a leaf: a list of (a list of a list of (a list of a quad and a sphere)
    and a triangle) -- a quad draw there takes 6 values, four child choices and
    its own two, the most an accepted tree draws -- and (a Transform over a
    list of a Transform over a moving sphere and a quad)."""
    c = s.Hittables()
    c.add(s.Quad((-2.9, 2.4, -0.6), (0.7, 0.1, 0.0), (0.0, 0.3, 0.9), m[0]))
    c.add(s.Sphere(*DEEP_SPHERE, m[1]))
    b = s.Hittables()
    b.add(c)
    b.add(s.Triangle((-1.9, 1.2, -1.4), (0.8, 0.0, 0.3), (0.1, 0.6, 0.2), m[2]))
    a = s.Hittables()
    a.add(b)
    q1 = rt.Quaternion.from_axis_angle(s.api, (0.2, -1.0, 0.7), 53.0)
    q2 = rt.Quaternion.from_axis_angle(s.api, (1.0, 0.4, 0.3), 118.0)
    d = s.Hittables()
    d.add(s.Transform(s.Sphere_new_with_motion((0.2, 0.1, -0.3), (0.5, 0.4, -0.3), 0.35, m[3]), (0.6, 0.9, 0.1), q2,
                      (1.4, 0.8, 1.1)))
    d.add(s.Quad((-0.5, 1.4, -0.4), (0.9, 0.0, 0.2), (0.1, 0.0, 0.8), m[4]))
    l = s.Hittables()
    l.add(a)
    l.add(s.Transform(d, (2.1, 1.3, -0.2), q1, (0.9, 1.5, 1.2)))
    return l


LEAVES = {"one_quad": 1, "one_sphere": 1, "one_triangle": 1, "flat": 3, "tree": 5, "deep": 5}
_LIGHTS = {"one_quad": _one_quad, "one_sphere": _one_sphere, "one_triangle": _one_triangle, "flat": _flat, "tree": _tree,
           "deep": _deep}
# name -> (box centre, box half-extent, the static sphere light origins go into, or None, the list sizes above it)
SETS = {
    "one_quad": ((0.0, 1.6, 0.0), 2.5, None, 1),
    "one_sphere": ((0.3, 1.8, -0.2), 2.5, SPHERE, 1),
    "one_triangle": ((0.0, 1.6, 0.0), 2.5, None, 1),
    "flat": ((0.0, 1.6, 0.0), 3.5, FLAT_SPHERE, 3),
    "tree": ((0.0, 1.8, 0.2), 3.5, TREE_SPHERE, 3),
    "deep": ((0.0, 1.8, 0.0), 3.5, DEEP_SPHERE, 2 * 1 * 2 * 2),
}


def build(rt, s, name):
    """(world, lights, cam) of a named light set on the scene's implementation."""
    m = [s.DiffuseLight(s.SolidColor((4.0 + k, 4.0, 4.0))) for k in range(LEAVES[name])]
    lights = _LIGHTS[name](rt, s, m)
    world = s.Hittables()
    world.add(s.Quad((-20.0, 0.0, -20.0), (40.0, 0.0, 0.0), (0.0, 0.0, 40.0), s.Lambertian(s.SolidColor((0.6, 0.6, 0.55)))))
    world.add(s.Sphere((-1.2, 0.5, 1.1), 0.5, s.Lambertian(s.SolidColor((0.7, 0.3, 0.2)))))
    world.add(s.Sphere((1.4, 0.6, -0.9), 0.6, s.Metal((0.8, 0.8, 0.9), 0.1)))
    world.add(_LIGHTS[name](rt, s, m))  # the lights' shapes as emitters
    cam = rt.Camera()
    cam.aspect_ratio = 1.0
    cam.image_width = 24
    cam.samples_per_pixel = 4
    cam.max_depth = 6
    cam.vertical_fov_in_degrees = 60.0
    cam.look_from, cam.look_at, cam.vec_up = (0.5, 1.5, 8.0), (0.0, 1.6, 0.0), (0.0, 1.0, 0.0)
    return world, lights, cam


def set_case(api, name):
    """(scene, world, lights, cam) of a named light set on `api`."""
    rt = pkg_module("raytracer")
    s = rt.Scene(api)
    return (s,) + build(rt, s, name)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    return set_case(driver(), name)


# ---------------------------------------------------------------- points
def _isotropic(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def origins_of(name):
    centre, half, sphere, _ = SETS[name]
    g = np.random.default_rng([POINT_SEED, sorted(SETS).index(name)])
    c = np.array(centre)
    o = c + g.uniform(-half, half, size=(N, 3))
    k = N - 16
    o[k:k + 8] = c + _isotropic(g, 8) * 1e3      # (the light sizes here are about 1)
    o[k + 8:k + 16] = c + _isotropic(g, 8) * 1e-3
    if sphere is not None:
        sc, sr = np.array(sphere[0]), sphere[1]
        k -= 65
        o[k:k + 64] = sc + _isotropic(g, 64) * sr * np.cbrt(g.uniform(1e-3, 0.97, size=(64, 1)))
        o[k + 64] = sc
    return np.ascontiguousarray(o), g


@functools.lru_cache(maxsize=None)
def reference(name):
    """(origins, dirs, pdf, samples) of a named light set, made once per
    process on the oracle and read-only: the point set, lights.pdf_value of it,
    and SAMPLES draws an origin at seed SEED.  Asserts what makes the set worth
    the query, from the oracle alone."""
    drv = driver()
    s, w, l, cam = oracle_case(name)
    o, g = origins_of(name)
    aim = oracle_sample(drv, s, l, o, 1, AIM_SEED)[:, 0]
    d = _isotropic(g, N)
    aimed = (np.arange(N) % 2 == 0) & (aim["flags"] == 0)
    d[aimed] = aim["dir"][aimed]
    d *= 10.0 ** g.uniform(-3.0, 3.0, size=(N, 1))
    d = np.ascontiguousarray(d)
    pdf = oracle_pdf(drv, s, l, o, d)
    smp = oracle_sample(drv, s, l, o, SAMPLES, SEED)
    nz, z = np.mean(pdf != 0), np.mean(pdf == 0)
    assert nz >= 0.25 and z >= 0.25, (name, nz, z)
    good = smp["flags"] == 0
    if SETS[name][2] is not None:
        # the origin at the sphere light's centre: every draw that chooses the sphere panics; so do those from inside it
        at_centre = good[N - 16 - 1]
        assert (~good).any() and (LEAVES[name] > 1 or not at_centre.any())
        # inside the sphere every direction hits it: the NaN branch's 1 / 4 pi, over the sizes of the lists above it
        inside = pdf[N - 16 - 65:N - 16 - 1]
        assert np.all(inside >= 1.0 / (4.0 * np.pi) / SETS[name][3] * (1.0 - 1e-15))
        assert LEAVES[name] > 1 or np.all(inside == 1.0 / (4.0 * np.pi))
    if LEAVES[name] > 1:
        leaf = oracle_leaf(drv, s, l, np.repeat(o, SAMPLES, axis=0)[good.reshape(-1)], smp["dir"][good])
        assert set(np.unique(leaf)) >= set(range(LEAVES[name])), (name, np.unique(leaf))
    for a in (o, d, pdf, smp):
        a.setflags(write=False)
    return o, d, pdf, smp
