"""Shared by tests/test_portal_cpu.py and tests/test_portal_gpu.py: the oracle
extended with the Portal material (tests/cpp/portal_oracle.cpp, which also
holds the Disney extension; built once per process as tests/disney_query.py
builds its driver) and the three render worlds.

A world is `build(s, portal=True) -> (world, lights, cam)`; with portal=False
every Portal is a Transparent (the twin world: the same handles in the same
order).  All frames are 32 x 18, 16 spp, depth 10.
"""
import ctypes as C
import functools
import os
import subprocess
import tempfile

from conftest import ROOT, pkg_module

WIDTH, SPP, DEPTH = 32, 16, 10
WHITE = (1.0, 1.0, 1.0)


@functools.lru_cache(maxsize=None)
def driver():
    """capi.Api of the oracle (on rt_crmath.h) with orc_mat_portal and orc_mat_disney bound."""
    capi = pkg_module("capi")
    out = os.path.join(tempfile.mkdtemp(prefix="portal_query_"), "libportal_oracle_cr.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DORC_CRMATH", "-shared", "-o", out,
           os.path.join(ROOT, "tests", "cpp", "portal_oracle.cpp"), os.path.join(ROOT, "oracle", "rt_oracle.cpp"),
           os.path.join(ROOT, "oracle", "rt_oracle_obj.cpp"), "-pthread", "-lz"]
    subprocess.run(cmd, check=True, timeout=600)
    api = capi.Api(C.CDLL(out), "orc_", capi.ORACLE_EXTRAS)
    for name in ("orc_mat_portal", "orc_mat_disney", "orc_disney_params_default"):
        assert name not in api.missing, name
    return api


def feature_bit(name):
    import re
    src = open(os.path.join(ROOT, "raytracer-2025_amd", "csrc", "rt_layout.h")).read()
    return int(re.search(r"\b%s = (\d+)u" % name, src).group(1))


# ---------------------------------------------------------------- worlds
def _camera(rt, look_from, look_at, fov, background=None):
    cam = rt.Camera()
    cam.aspect_ratio = 16 / 9
    cam.image_width = WIDTH
    cam.samples_per_pixel = SPP
    cam.max_depth = DEPTH
    cam.vertical_fov_in_degrees = fov
    cam.look_from, cam.look_at, cam.vec_up = look_from, look_at, (0.0, 1.0, 0.0)
    if background is not None:
        cam.background = background
    return cam


def _portal(s, portal, attenuation, offset=None, rotation=None):
    return s.Portal(attenuation, offset, rotation) if portal else s.Transparent()


def world_scene(s, portal=True, null_portal=False):
    """scenes.portal_scene: the reference's quad, sphere, camera and ACES tone
    map under the sky gradient.  null_portal: Portal(WHITE, 0, identity) in the
    quad's place, which must render as Transparent does."""
    scenes = pkg_module("scenes")
    rt = pkg_module("raytracer")
    mat = None
    if null_portal:
        mat = s.Portal(WHITE, (0.0, 0.0, 0.0), rt.Quaternion.identity())
    elif not portal:
        mat = s.Transparent()
    return scenes.portal_scene(s, image_width=WIDTH, samples_per_pixel=SPP, max_depth=DEPTH, quad_material=mat)


def world_rotated(s, portal=True):
    """A five-quad box with a quad light passed as `lights` (a Portal hit is
    the Ray arm: no mixture draw), a tinted rotating Portal on a sphere inside
    a BVH, a Portal with a non-unit quaternion on a triangle under a
    Transform, and a moving sphere behind them (the carried time)."""
    rt = pkg_module("raytracer")
    red = s.Lambertian(s.SolidColor((0.65, 0.05, 0.05)))
    white = s.Lambertian(s.SolidColor((0.73, 0.73, 0.73)))
    green = s.Lambertian(s.SolidColor((0.12, 0.45, 0.15)))
    light = s.DiffuseLight(s.SolidColor((15.0, 15.0, 15.0)))
    tinted = _portal(s, portal, (0.9, 0.7, 0.5), (35.0, 20.0, 60.0),
                     rt.Quaternion.from_axis_angle(s.api, (0.3, 1.0, 0.2), 37.0))
    skewed = _portal(s, portal, (0.95, 0.95, 0.95), (-20.0, 30.0, 10.0), rt.Quaternion(0.5, 0.5, 0.5, 0.7))
    w = s.Hittables()
    w.add(s.Quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green))
    w.add(s.Quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red))
    w.add(s.Quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white))
    w.add(s.Quad((555, 555, 555), (-555, 0, 0), (0, 0, -555), white))
    w.add(s.Quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white))
    w.add(s.Quad((183, 554, 177), (190, 0, 0), (0, 0, 205), light))
    objs = s.Hittables()
    objs.add(s.Sphere((170, 100, 170), 100, tinted))
    objs.add(s.Sphere((430, 60, 110), 60, white))
    objs.add(s.Sphere((80, 40, 60), 40, green))
    objs.add(s.Sphere((500, 35, 300), 35, red))
    w.add(s.BVH(objs))
    tri = s.Triangle((-110, 20, 0), (220, 0, -40), (60, 260, 30), skewed)
    w.add(s.Transform(tri, (390, 0, 300), rt.Quaternion.from_axis_angle(s.api, (0, 1, 0), 18.0), None))
    w.add(s.Sphere_new_with_motion((278, 150, 460), (278, 230, 460), 70, white))
    lights = s.Hittables()
    lights.add(s.Quad((183, 554, 177), (190, 0, 0), (0, 0, 205), s.EmptyMaterial()))
    return w, lights, _camera(rt, (278.0, 278.0, -800.0), (278.0, 278.0, 0.0), 40.0)


def world_wrapped(s, portal=True):
    """Mix(portal, Lambertian, 0.5), DiffuseLight(tex, portal) and a Disney
    sphere under a sky gradient; two Portal quads facing the camera whose
    offsets lead in front of each other, so that a path bounces between them
    until max_depth ends it; and a Portal quad whose offset leads inside a
    ConstantMedium."""
    rt = pkg_module("raytracer")
    w = s.Hittables()
    w.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))))
    turn = _portal(s, portal, (0.8, 0.9, 1.0), (0.0, 0.5, 0.0), rt.Quaternion.from_axis_angle(s.api, (0, 1, 0), 25.0))
    w.add(s.Sphere((-2.3, 1.0, 0.0), 1.0, s.Mix(turn, s.Lambertian(s.SolidColor((0.7, 0.3, 0.3))), 0.5)))
    shift = _portal(s, portal, (0.9, 0.9, 0.9), (0.3, 0.0, 0.0), None)
    w.add(s.Sphere((0.0, 1.0, 0.4), 1.0, s.DiffuseLight(s.SolidColor((0.4, 0.3, 0.1)), shift)))
    w.add(s.Sphere((2.3, 1.0, 0.0), 1.0, s.Disney(s.SolidColor((0.7, 0.1, 0.1)), clearcoat=1.0, clearcoat_gloss=0.5)))
    # the pair: a ray travelling -z meets `near` (z = 1), leaves at z = -0.5, meets `far` (z = -1), leaves at
    # z = 1.5 in front of `near` again
    near = _portal(s, portal, (0.97, 0.97, 0.97), (0.0, 0.0, -1.5), None)
    far = _portal(s, portal, (0.97, 0.97, 0.97), (0.0, 0.0, 2.5), None)
    w.add(s.Quad((-4.5, 2.2, 1.0), (1.5, 0.0, 0.0), (0.0, 1.2, 0.0), near))
    w.add(s.Quad((-4.5, 2.2, -1.0), (1.5, 0.0, 0.0), (0.0, 1.2, 0.0), far))
    # into the fog: the quad's centre (3.75, 2.8, 1) is taken to the medium's centre
    fog = s.ConstantMedium(s.Sphere((4.2, 0.8, 1.5), 0.7, s.EmptyMaterial()), 0.8, s.SolidColor((0.9, 0.9, 0.9)))
    w.add(fog)
    into = _portal(s, portal, (1.0, 0.95, 0.9), (0.45, -2.0, 0.5), None)
    w.add(s.Quad((3.0, 2.2, 1.0), (1.5, 0.0, 0.0), (0.0, 1.2, 0.0), into))
    return w, None, _camera(rt, (0.0, 2.5, 9.0), (0.0, 1.4, 0.0), 38.0, s.SkyGradient())


WORLDS = {"scene": world_scene, "rotated": world_rotated, "wrapped": world_wrapped}
TIERS = {"scene": 4, "rotated": 4, "wrapped": 5}


@functools.lru_cache(maxsize=None)
def reference(name, seed=1, **variant):
    """The driver's render of a named world, made once per process:
    (linear, srgb, partials, panics)."""
    rt = pkg_module("raytracer")
    s = rt.Scene(driver())
    world, lights, cam = WORLDS[name](s, **variant)
    lin, srgb, st = cam.render(world, lights, seed=seed)
    part, _ = cam.render_partials(world, lights, seed=seed)
    for a in (lin, srgb, part):
        a.setflags(write=False)
    return lin, srgb, part, int(st.panics)
