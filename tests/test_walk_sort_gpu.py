"""The basic tier's packed-word child sort on the GPU against the oracle: a
node visit of the 4-wide walk sorts its hit box children as 32-bit words -- the
upper 16 bits of the f32 entry distance above the 16-bit ref code -- and pushes
them rotated into stack entries (raytracer-2025_amd/csrc/rt_sort4.h,
rt_walk4.h visit4_rows; the words themselves: tests/test_sort4_cpu.py).
Children whose distances agree in their upper 16 bits are walked in the order
of their ref codes, not of their distances; the closest hit does not depend on
the order of the visits, so no sample may change: the f32 frames are equal to
the oracle's (RMSE 0) and no (pixel, stratum row) sum diverges.  Frames of
48x27 pixels, 4 spp, depth 8, on the product and on the check build.

(a) a 5x5x5 lattice of equal spheres seen along an axis from a lattice plane:
    sibling boxes with equal entry distances, exact ties in the sort;
(b) the same lattice seen along its diagonal: near-equal entry distances,
    equal in their upper 16 bits or a step apart;
(c) the lattice as one child of a Hittables beside two loose spheres: the list
    walk's own stack entries (the "next list position" push) and list-element
    spheres queued with their flag bit, between the sorted pushes;
(d) 17 spheres on a line along the view axis: a narrow tree (six 4-wide nodes)
    whose boxes a ray enters one behind the other, so the sorted order is the
    order along the ray and the farther children wait on the stack;
(e) about 900 spheres: a tree of more than 365 nodes, which the basic tier's
    wide variant (rt_path_kernel<0, true>) runs.
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import divergence, rmse_per_channel
from test_parity_gpu import gpu_partials

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")


def _camera(rt, s, look_from, look_at, fov=40.0):
    cam = rt.Camera()
    cam.aspect_ratio = 16 / 9
    cam.image_width = 48
    cam.samples_per_pixel = 4
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


def _lattice(s, mats):
    objs = s.Hittables()
    k = 0
    for x in range(-2, 3):
        for y in range(-2, 3):
            for z in range(-2, 3):
                objs.add(s.Sphere((float(x), float(y), float(z)), 0.25, mats[k % 4]))
                k += 1
    return objs


def world_axis(rt, s):
    w = s.Hittables()
    w.add(s.BVH(_lattice(s, _mats(s))))
    return w, None, _camera(rt, s, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0))


def world_diagonal(rt, s):
    w = s.Hittables()
    w.add(s.BVH(_lattice(s, _mats(s))))
    return w, None, _camera(rt, s, (6.0, 6.0, 6.0), (0.0, 0.0, 0.0))


def world_list(rt, s):
    mats = _mats(s)
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, 4.0), 0.5, mats[1]))  # glass, between the camera and the lattice
    w.add(s.BVH(_lattice(s, mats)))
    w.add(s.Sphere((0.0, -1003.0, 0.0), 1000.0, mats[3]))
    return w, None, _camera(rt, s, (0.5, 0.0, 9.0), (0.0, 0.0, 0.0))


def world_line(rt, s):
    mats = _mats(s)
    objs = s.Hittables()
    for i in range(17):
        objs.add(s.Sphere((0.02 * i, 0.0, -1.5 * i), 0.6, mats[i % 4]))
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w, None, _camera(rt, s, (0.4, 0.5, 6.0), (0.0, 0.0, -6.0), fov=25.0)


def world_many(rt, s, n=880):
    import random
    rnd = random.Random(n)
    mats = _mats(s)
    objs = s.Hittables()
    objs.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, mats[3]))
    for i in range(n):
        objs.add(s.Sphere((rnd.uniform(-4, 4), 0.1, rnd.uniform(-6, 3)), 0.1, mats[i % 4]))
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w, None, _camera(rt, s, (0.0, 1.0, 6.0), (0.0, 0.3, 0.0))


WORLDS = {"axis": world_axis, "diagonal": world_diagonal, "list": world_list, "line": world_line,
          "many": world_many}


def _render(api, rt, build, on_gpu):
    scene = rt.Scene(api)
    world, lights, cam = build(scene)
    lin, _, st = cam.render(world, lights, seed=1)
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
def test_sorted_walk_equals_the_oracle(builds, oracle_frames, rt, capi, name, build):
    api = builds[build]
    make = lambda s: WORLDS[name](rt, s)
    g, gpart, gst = _render(api, rt, make, True)
    o, opart, ost = oracle_frames(name)
    assert g.shape == o.shape == (27, 48, 3)
    assert gst.panics == 0 and ost.panics == 0
    div = divergence(gpart, opart)
    rmse = rmse_per_channel(g, o)
    differing = int(np.any(g != o, axis=-1).sum())
    print(f"{name} / {build}: per-channel RMSE {rmse}, pixels differing from the oracle {differing}, "
          f"diverged (pixel, s_i) sums {div}")
    # every world runs the basic tier; "many" its wide variant (more nodes than
    # the batch variant's LDS copy holds: RT_NODE_LDS_BATCH_BYTES / 112 = 365)
    s = rt.Scene(api)
    w, _, cam = make(s)
    info = capi.RtWorldInfo()
    assert api.world_info_get(s.s, w.h, -1, cam.background.h, 0, ctypes.byref(info)) == 0
    assert info.kernel_tier == 0
    assert (info.bvh_nodes > 365) == (name == "many"), info.bvh_nodes
    assert np.all(rmse == 0.0), rmse
    np.testing.assert_array_equal(g, o)
    assert div == 0
