"""The rebuilt trees on the GPU against the oracle: the flatten's SAH build
splits small ranges by a full sweep and the 4-wide collapse picks the cut of
least cost (raytracer-2025_amd/csrc/rt_scene.cpp sah_build, bvh4_collapse), so
every world's tree differs from the one the kernels walked before -- and any
BVH over the same leaves finds the same closest hit.  Frames of 64x36 pixels at
4 spp are equal to the oracle's (RMSE 0, every f32 equal, no (pixel, stratum
row) sum diverged, no panic), on the product and on the check build, for:

(a) the C2 world (book-1 random spheres, 485 leaves);
(b) sphere worlds of 1, 2, 3 and 5 spheres under a BVH;
(c) spheres with coincident centres (glass shells round a core): no split
    separates them, the build falls back to the median;
(d) 2049 small spheres and the ground: one binned range over swept ones, and
    more nodes than the basic tier's LDS copy holds (the mesh tier walks them);
(e) a small terrain OBJ (mesh tier: triangles in per-model BVHs);
(f) the C5 scene (full tier: boxes, a Transform over a sphere BVH, media).

And rt_world_hit on the C2 world gives the records of the oracle's
Hittable::hit driver (tests/hit_query.py) for that world's ray set."""
import ctypes
import os
import random

import numpy as np
import pytest

from conftest import divergence, rmse_per_channel
from test_parity_gpu import gpu_partials
import hit_query as hq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")
W, SPP = 64, 4


def _camera(rt, s, look_from, look_at, fov=40.0):
    cam = rt.Camera()
    cam.aspect_ratio = 16 / 9
    cam.image_width = W
    cam.samples_per_pixel = SPP
    cam.max_depth = 8
    cam.vertical_fov_in_degrees = fov
    cam.look_from = look_from
    cam.look_at = look_at
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.background = s.SkyGradient()
    return cam


def _mats(s):
    return [s.Lambertian(s.SolidColor((0.8, 0.3, 0.2))), s.Dielectric(s.SolidColor((1.0, 1.0, 1.0)), 1.5),
            s.Metal((0.7, 0.6, 0.5), 0.0), s.Lambertian(s.SolidColor((0.2, 0.5, 0.7)))]


def _under_bvh(s, objs):
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w


def world_few(n):
    def build(rt, scenes, s, tmp):
        mats = _mats(s)
        objs = s.Hittables()
        for i in range(n):
            objs.add(s.Sphere((-2.0 + 1.3 * i, 0.3 * (i % 2), -0.4 * i), 0.55, mats[i % 4]))
        return _under_bvh(s, objs), None, _camera(rt, s, (0.7, 1.1, 7.0), (0.6, 0.1, -0.5))
    return build


def world_coincident(rt, scenes, s, tmp):
    mats = _mats(s)
    objs = s.Hittables()
    for i in range(6):  # glass shells round a diffuse core: every centre and every centroid equal
        objs.add(s.Sphere((0.0, 0.0, 0.0), 0.4 + 0.25 * i, mats[1] if i else mats[0]))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 0.6, 6.0), (0.0, 0.0, 0.0))


def world_2049(rt, scenes, s, tmp):
    rng = random.Random(11)
    mats = _mats(s)
    objs = s.Hittables()
    for i in range(2049):
        objs.add(s.Sphere((rng.uniform(-12, 12), 0.12, rng.uniform(-12, 12)), 0.12, mats[i % 4]))
    objs.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, mats[3]))
    return _under_bvh(s, objs), None, _camera(rt, s, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), fov=30.0)


def world_c2(rt, scenes, s, tmp):
    return scenes.random_spheres(s, W, SPP)


def world_terrain(rt, scenes, s, tmp):
    path = os.path.join(tmp, "terrain.obj")
    if not os.path.exists(path):
        scenes.write_terrain_obj(tmp, 24)
    return scenes.obj_terrain(s, path, W, SPP)


def world_c5(rt, scenes, s, tmp):
    return scenes.final_scene(s, W, SPP, 40, aspect_ratio=16 / 9)


# name -> (build, kernel tier)
WORLDS = {"c2": (world_c2, 0), "one": (world_few(1), 0), "two": (world_few(2), 0), "three": (world_few(3), 0),
          "five": (world_few(5), 0), "coincident": (world_coincident, 0), "spheres2049": (world_2049, 1),
          "terrain": (world_terrain, 1), "c5": (world_c5, 2)}


@pytest.fixture(scope="module")
def builds(capi, gpu):
    # the check build is a build product (__graft_entry__.build() makes it): absent is a failure
    assert os.path.exists(CHECK_SO), "check build absent: make -C raytracer-2025_amd check (__graft_entry__.build())"
    chk = capi.Api(ctypes.CDLL(CHECK_SO), "rt_")
    assert not chk.missing, chk.missing
    return {"product": gpu, "check": chk}


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return str(tmp_path_factory.mktemp("tree_worlds"))


def _render(api, rt, scenes, name, tmp, on_gpu):
    scene = rt.Scene(api)
    world, lights, cam = WORLDS[name][0](rt, scenes, scene, tmp)
    lin, _, st = cam.render(world, lights, seed=1)  # raises on a check failure (RT_EPANIC)
    if on_gpu:
        part = gpu_partials(api, scene, cam, lin.shape[0])
    else:
        part, _ = cam.render_partials(world, lights, seed=1)
    return lin, part, st


@pytest.fixture(scope="module")
def oracle_frames(oracle, rt, scenes, tmp):
    """Each world's oracle frame, rendered once for both builds."""
    frames = {}

    def get(name):
        if name not in frames:
            frames[name] = _render(oracle, rt, scenes, name, tmp, False)
        return frames[name]
    return get


@pytest.mark.parametrize("build", ["product", "check"])
@pytest.mark.parametrize("name", sorted(WORLDS))
def test_rebuilt_tree_renders_the_oracle_frame(builds, oracle_frames, rt, scenes, capi, tmp, name, build):
    api = builds[build]
    g, gpart, gst = _render(api, rt, scenes, name, tmp, True)
    o, opart, ost = oracle_frames(name)
    assert g.shape == o.shape == (36, 64, 3)
    div = divergence(gpart, opart)
    rmse = rmse_per_channel(g, o)
    differing = int(np.any(g != o, axis=-1).sum())
    s = rt.Scene(api)
    w, lights, cam = WORLDS[name][0](rt, scenes, s, tmp)
    info = capi.RtWorldInfo()
    assert api.world_info_get(s.s, w.h, -1 if lights is None else lights.h, cam.background.h if cam.background else -1, 0,
                              ctypes.byref(info)) == 0
    print(f"{name} / {build}: tier {info.kernel_tier}, {info.bvh_nodes} nodes, stack need {info.stack_need}; per-channel "
          f"RMSE {rmse}, pixels differing from the oracle {differing}, diverged (pixel, s_i) sums {div}")
    assert info.kernel_tier == WORLDS[name][1]
    assert gst.panics == 0 and ost.panics == 0
    assert np.all(rmse == 0.0), rmse
    np.testing.assert_array_equal(g, o)
    assert div == 0


@pytest.mark.parametrize("build", ["product", "check"])
def test_world_hit_on_the_c2_world_equals_the_driver(builds, rt, scenes, build):
    drv = hq.driver(True)
    so = rt.Scene(drv)
    wo, _, camo = scenes.random_spheres(so, W, SPP)
    # (a point in the metal ball, a point in the glass one off its centre)
    extras = {"inside": [(4.0, 1.0, 0.0), (0.05, 1.03, -0.04)]}
    rays, where = hq.ray_set(lambda r: hq.oracle_hit(drv, so, wo, r, 0), camo, extras)
    ref = hq.oracle_hit(drv, so, wo, rays, 0)
    s = rt.Scene(builds[build])
    w, _, _ = scenes.random_spheres(s, W, SPP)
    got = s.hit(w, rays, seed=0, flags=0)
    gb, rb = hq.geometry_bytes(got), hq.geometry_bytes(ref)
    bad = np.nonzero(np.any(gb != rb, axis=1))[0]
    print(f"c2 / {build}: {len(rays)} rays, {int(((ref['flags'] & hq.FOUND) != 0).sum())} hits, "
          f"{len(bad)} records differ from the driver")
    assert len(rays) > 3000 and ((ref["flags"] & hq.FOUND) != 0).sum() > 1000
    assert np.array_equal(gb, rb)
