"""The basic tier's sign-ordered slab test on the GPU against the oracle: a
lane reads each axis' near and far row of a node from the block's LDS copy at
an address offset by the sign of its ray's 1/d, and the visit tests the slots
with slab_sorted_f -- the six plane distances of slab_f without the per-axis
min / max (raytracer-2025_amd/csrc/rt_slab.h, rt_walk4.h load_node4_sorted
and visit4_rows; the test itself on CPU: tests/test_slab_sorted_cpu.py).  The
walk must visit the same nodes in the same order, so no sample may change: the
f32 frames are equal to the oracle's (RMSE 0), no (pixel, stratum row) sum
diverges and the render reports no error -- on the product and on the check
build, whose visit runs slab_f beside every slab_sorted_f and fails the render
when a verdict, or the entry of a hit, differs.  Frames of 32x18 pixels,
4 spp (the ~900-sphere world: 16), depth 8.

(a) six axis views: the camera's axes exactly along +-x, +-y, +-z over a
    4x4x4 lattice of spheres, 8 in each octant -- every sign pattern of 1/d,
    and direction components at and next to zero around the frame's centre;
(b) boxes behind the origin: a camera beyond every lattice sphere looking away
    from them over the ground, and one looking across them;
(c) glass: the camera inside a Dielectric sphere that holds another, beside
    more glass -- rays that start inside the boxes they test;
(d) a 5x5x5 lattice seen along its diagonal: a tree four levels deep;
(e) the 904-sphere world of scripts/sphere_scaling.py: more nodes than the
    batch variant's LDS copy holds, so the wide variant (rt_path_kernel<0,
    true>) runs.
"""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import divergence, rmse_per_channel
from test_parity_gpu import gpu_partials

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")


def _camera(rt, s, look_from, look_at, vec_up=(0.0, 1.0, 0.0), fov=40.0, spp=4):
    cam = rt.Camera()
    cam.aspect_ratio = 16 / 9
    cam.image_width = 32
    cam.samples_per_pixel = spp
    cam.max_depth = 8
    cam.vertical_fov_in_degrees = fov
    cam.look_from = look_from
    cam.look_at = look_at
    cam.vec_up = vec_up
    cam.background = s.SkyGradient()
    return cam


def _mats(s):
    return [s.Lambertian(s.SolidColor((0.8, 0.3, 0.2))), s.Dielectric(s.SolidColor((1.0, 1.0, 1.0)), 1.5),
            s.Metal((0.7, 0.6, 0.5), 0.0), s.Lambertian(s.SolidColor((0.2, 0.5, 0.7)))]


def _lattice(s, mats, coords, r):
    objs = s.Hittables()
    k = 0
    for x in coords:
        for y in coords:
            for z in coords:
                objs.add(s.Sphere((x, y, z), r, mats[k % 4]))
                k += 1
    return objs


def _under_bvh(s, objs):
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w


OCTANTS = (-2.25, -0.75, 0.75, 2.25)  # 4x4x4: eight spheres in every octant


def world_view(axis, sign):
    def build(rt, s):
        w = _under_bvh(s, _lattice(s, _mats(s), OCTANTS, 0.5))
        eye = [0.0, 0.0, 0.0]
        eye[axis] = 9.0 * sign
        up = (0.0, 0.0, 1.0) if axis == 1 else (0.0, 1.0, 0.0)
        return w, None, _camera(rt, s, tuple(eye), (0.0, 0.0, 0.0), vec_up=up)
    return build


def _grounded_lattice(s):
    objs = _lattice(s, _mats(s), OCTANTS, 0.5)
    objs.add(s.Sphere((0.0, -1003.0, 0.0), 1000.0, _mats(s)[3]))
    return _under_bvh(s, objs)


def world_behind_away(rt, s):
    return _grounded_lattice(s), None, _camera(rt, s, (0.0, 0.0, 12.0), (0.0, -1.0, 30.0))


def world_behind_across(rt, s):
    return _grounded_lattice(s), None, _camera(rt, s, (0.0, 0.0, 12.0), (30.0, -1.0, 12.5), fov=70.0)


def world_glass(rt, s):
    mats = _mats(s)
    objs = s.Hittables()
    objs.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, mats[3]))
    objs.add(s.Sphere((0.0, 1.0, 6.0), 3.0, mats[1]))  # the camera is inside it
    objs.add(s.Sphere((0.3, 1.2, 4.5), 0.8, mats[1]))  # glass inside the glass
    for i in range(8):
        objs.add(s.Sphere((-3.5 + i, 0.5, 0.5 * (i % 2)), 0.5, mats[1 if i % 2 else i % 4]))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 1.0, 6.0), (0.0, 0.4, 0.0))


def world_deep(rt, s):
    w = _under_bvh(s, _lattice(s, _mats(s), (-2.0, -1.0, 0.0, 1.0, 2.0), 0.25))
    return w, None, _camera(rt, s, (6.0, 6.0, 6.0), (0.0, 0.0, 0.0))


def world_wide(rt, s, n=900):
    """scripts/sphere_scaling.py's world of n + 4 spheres under the book-1 camera's view"""
    from conftest import pkg_module
    g = pkg_module("scenes").SplitMix64(7)
    objs = s.Hittables()
    objs.add(s.Sphere((0, -1000, 0), 1000, s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))))
    side = int(math.ceil(math.sqrt(n)))
    half = side / 2.0
    cell = 22.0 / max(side, 22) if side > 22 else 1.0
    k = 0
    for a in range(side):
        for b in range(side):
            if k >= n:
                break
            k += 1
            cm = g.f64()
            c = ((a - half) * cell + 0.9 * cell * g.f64(), 0.2, (b - half) * cell + 0.9 * cell * g.f64())
            r = 0.2 * min(1.0, cell)
            if cm < 0.8:
                mat = s.Lambertian(s.SolidColor((g.f64() * g.f64(), g.f64() * g.f64(), g.f64() * g.f64())))
            elif cm < 0.95:
                mat = s.Metal((g.range(0.5, 1), g.range(0.5, 1), g.range(0.5, 1)), g.range(0, 0.5))
            else:
                mat = s.Dielectric(s.SolidColor((1, 1, 1)), 1.5)
            objs.add(s.Sphere((c[0], r, c[2]), r, mat))
    objs.add(s.Sphere((0, 1, 0), 1.0, s.Dielectric(s.SolidColor((1, 1, 1)), 1.5)))
    objs.add(s.Sphere((-4, 1, 0), 1.0, s.Lambertian(s.SolidColor((0.4, 0.2, 0.1)))))
    objs.add(s.Sphere((4, 1, 0), 1.0, s.Metal((0.7, 0.6, 0.5), 0.0)))
    return _under_bvh(s, objs), None, _camera(rt, s, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), fov=20.0, spp=16)


WORLDS = {"view+x": world_view(0, 1.0), "view-x": world_view(0, -1.0), "view+y": world_view(1, 1.0),
          "view-y": world_view(1, -1.0), "view+z": world_view(2, 1.0), "view-z": world_view(2, -1.0),
          "behind_away": world_behind_away, "behind_across": world_behind_across, "glass": world_glass,
          "deep": world_deep, "wide": world_wide}


def _render(api, rt, build, on_gpu):
    scene = rt.Scene(api)
    world, lights, cam = build(scene)
    lin, _, st = cam.render(world, lights, seed=1)  # raises on a check failure (RT_EPANIC)
    if on_gpu:
        part = gpu_partials(api, scene, cam, lin.shape[0])
    else:
        part, _ = cam.render_partials(world, lights, seed=1)
    return lin, part, st


@pytest.fixture(scope="module")
def oracle_frames(oracle, rt):
    """Each world's oracle frame, rendered once for both builds."""
    frames = {}

    def get(name):
        if name not in frames:
            frames[name] = _render(oracle, rt, lambda s: WORLDS[name](rt, s), False)
        return frames[name]
    return get


@pytest.fixture(scope="module")
def builds(capi, gpu):
    # the check build is a build product (__graft_entry__.build() makes it): absent is a failure
    assert os.path.exists(CHECK_SO), "check build absent: make -C raytracer-2025_amd check (__graft_entry__.build())"
    chk = capi.Api(ctypes.CDLL(CHECK_SO), "rt_")
    assert not chk.missing, chk.missing
    return {"product": gpu, "check": chk}


@pytest.mark.parametrize("build", ["product", "check"])
@pytest.mark.parametrize("name", sorted(WORLDS))
def test_sign_ordered_walk_equals_the_oracle(builds, oracle_frames, rt, capi, name, build):
    api = builds[build]
    make = lambda s: WORLDS[name](rt, s)
    g, gpart, gst = _render(api, rt, make, True)
    o, opart, ost = oracle_frames(name)
    assert g.shape == o.shape == (18, 32, 3)
    assert gst.panics == 0 and ost.panics == 0
    div = divergence(gpart, opart)
    rmse = rmse_per_channel(g, o)
    differing = int(np.any(g != o, axis=-1).sum())
    print(f"{name} / {build}: per-channel RMSE {rmse}, pixels differing from the oracle {differing}, "
          f"diverged (pixel, s_i) sums {div}")
    # every world runs the basic tier; "wide" its wide variant (more nodes than
    # the batch variant's LDS copy holds: RT_NODE_LDS_BATCH_BYTES / 112 = 365);
    # more than 1 + 4 nodes are a tree three levels deep
    s = rt.Scene(api)
    w, _, cam = make(s)
    info = capi.RtWorldInfo()
    assert api.world_info_get(s.s, w.h, -1, cam.background.h, 0, ctypes.byref(info)) == 0
    assert info.kernel_tier == 0
    assert (info.bvh_nodes > 365) == (name == "wide"), info.bvh_nodes
    if name == "deep":
        assert info.bvh_nodes > 5, info.bvh_nodes
    assert np.all(rmse == 0.0), rmse
    np.testing.assert_array_equal(g, o)
    assert div == 0
