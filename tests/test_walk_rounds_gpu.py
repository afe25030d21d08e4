"""The basic tier's walk loop and its sphere-round decision on the GPU against
the oracle.  The batch loop of rt_path_kernel<0, false>
(raytracer-2025_amd/csrc/rt_kernel_path.hip) calls trace4_step with every lane of
the wave in uniform control flow: a lane whose walk is over, or that has no
path, holds the empty state and must do nothing there; the step counts the
lanes in the walk from the state itself (a word to walk or a sphere queued)
and decides the round on that count -- no lane can walk on, or as many lanes
as the threshold asks hold a queued sphere.  The decisions must be the ones
taken when only walking lanes entered the step: every lane visits the same
nodes and tests the same spheres in the same order, so no sample may change.
The f32 frames are equal to the oracle's (RMSE 0), no (pixel, stratum row)
sum diverges and the render reports no error -- on the product and on the
check build, whose visit runs slab_f beside every slab_sorted_f.  Frames of
32x18 pixels, 4 spp (the ~900-sphere world: 16), depth 8; the thin frames 8x4
pixels, 1 spp.

Each world drives one edge of the decision:

(a) sparse: a BVH of four small spheres far apart, a mirror ball inside the
    glass one -- few lanes ever hold a queued sphere, so the rounds are those
    of a wave none of whose lanes can walk on, and most lanes of a wave are
    between walks while a few walk;
(b) nested: twelve heavily overlapping spheres at the frame's centre, glass
    outside and opaque inside -- a central ray hits more boxes than a lane's
    queue holds (RT_PEND_CAP = 8), lanes wait with a full queue, and steps
    with and without a round alternate;
(c) lattice: 5x5x5 spheres with glass among them over a ground sphere -- walks
    parked across shading rounds resume beside lanes that begin theirs;
(d) (a) - (c), (e) and (h) as thin frames: 32 queue entries, so half the wave's
    lanes never have a path, and fewer lanes in the walk than RT_DEFER_THIN,
    so the threshold is one lane;
(e) mixed: a Hittables holding two standalone spheres, a nested Hittables and
    a BVH, rendered with RT_FLAG_REFERENCE_BVH -- the flatten then keeps the
    list (by default it rebuilds a list that holds a BVH as one BVH over its
    elements, and the kernel would see the world of (f)): list positions,
    sphere words and nodes among one wave's walk words, so that lanes at a
    node, lanes waiting for their round and idle lanes are in the wave when
    the step's list block runs;
(f) mixed_bvh: the spheres of (e) under one BVH -- walk words that are nodes
    only;
(h) listed: the same spheres in a Hittables of two spheres and a nested
    Hittables, no BVH anywhere -- the flatten keeps such lists as they are
    (no 4-wide node at all): every walk word is a list position or a sphere;
(g) wide: the 904-sphere world of scripts/sphere_scaling.py -- more nodes
    than the batch variant's LDS copy holds, so rt_path_kernel<0, true> runs
    the whole-wave loop, in which only walking lanes take the step.

tests/test_walk_rounds_cpu.py holds the worlds to what they are meant to be
on the oracle alone: sphere hits and sky misses in every frame, glass
scatters and paths cut at the depth limit in the full frames.
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

FULL = {"width": 32, "aspect": 16 / 9, "spp": 4}  # 32x18
THIN = {"width": 8, "aspect": 2.0, "spp": 1}      # 8x4: 32 queue entries


def _camera(rt, s, look_from, look_at, fov, width, aspect, spp):
    cam = rt.Camera()
    cam.aspect_ratio = aspect
    cam.image_width = width
    cam.samples_per_pixel = spp
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


def world_sparse(rt, s, frame):
    mats = _mats(s)
    objs = s.Hittables()
    # a mirror ball inside dense glass (total reflection past 25 degrees): paths that stay in there
    objs.add(s.Sphere((-3.6, 1.3, 0.0), 1.3, s.Dielectric(s.SolidColor((1.0, 1.0, 1.0)), 2.4)))
    objs.add(s.Sphere((-3.6, 1.3, 0.0), 0.9, mats[2]))
    objs.add(s.Sphere((3.6, -1.3, -1.0), 1.2, mats[0]))
    objs.add(s.Sphere((-0.8, -1.9, 2.0), 1.0, mats[2]))
    objs.add(s.Sphere((1.2, 1.9, -2.0), 1.0, mats[1]))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), 40.0, **frame)


def world_nested(rt, s, frame):
    mats = _mats(s)
    objs = s.Hittables()
    for i in range(12):  # radii 2.0 down to 0.35, the centres a little apart: glass shells round an opaque core
        r = 2.0 - 0.15 * i
        objs.add(s.Sphere((0.02 * i, 0.015 * i, -0.01 * i), r, mats[1] if i < 9 else mats[i % 4]))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), 40.0, **frame)


def world_lattice(rt, s, frame):
    mats = _mats(s)
    objs = s.Hittables()
    k = 0
    for x in (-2.0, -1.0, 0.0, 1.0, 2.0):
        for y in (-2.0, -1.0, 0.0, 1.0, 2.0):
            for z in (-2.0, -1.0, 0.0, 1.0, 2.0):
                objs.add(s.Sphere((x, y, z), 0.3, mats[k % 4]))
                k += 1
    objs.add(s.Sphere((0.0, -1003.0, 0.0), 1000.0, mats[3]))
    return _under_bvh(s, objs), None, _camera(rt, s, (6.0, 5.0, 7.0), (0.0, 0.0, 0.0), 40.0, **frame)


def _mixed_spheres(s):
    """(standalone, listed, under the BVH): the spheres of the mixed worlds"""
    mats = _mats(s)
    alone = [((-2.6, 0.0, 0.0), 1.0, mats[1]), ((2.6, 0.4, -1.0), 1.0, mats[2])]
    # (the second one a mirror ball inside the standalone glass sphere)
    listed = [((0.0, 1.9, 0.0), 0.7, mats[0]), ((-2.6, 0.0, 0.0), 0.5, mats[2]), ((0.0, -1.9, 0.5), 0.7, mats[1])]
    tree = [((-1.2 + 0.6 * (i % 5), 0.6 * (i // 5) - 0.3, 1.0 - 0.5 * (i % 2)), 0.35, mats[i % 4]) for i in range(10)]
    return alone, listed, tree


def world_mixed(rt, s, frame):
    alone, listed, tree = _mixed_spheres(s)
    w = s.Hittables()
    w.add(s.Sphere(*alone[0]))
    inner = s.Hittables()
    for sp in listed:
        inner.add(s.Sphere(*sp))
    w.add(inner)
    objs = s.Hittables()
    for sp in tree:
        objs.add(s.Sphere(*sp))
    w.add(s.BVH(objs))
    w.add(s.Sphere(*alone[1]))
    return w, None, _camera(rt, s, (0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 40.0, **frame)


def world_listed(rt, s, frame):
    alone, listed, tree = _mixed_spheres(s)
    w = s.Hittables()
    w.add(s.Sphere(*alone[0]))
    inner = s.Hittables()
    for sp in listed + tree:
        inner.add(s.Sphere(*sp))
    w.add(inner)
    w.add(s.Sphere(*alone[1]))
    return w, None, _camera(rt, s, (0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 40.0, **frame)


def world_mixed_bvh(rt, s, frame):
    alone, listed, tree = _mixed_spheres(s)
    objs = s.Hittables()
    for sp in alone + listed + tree:
        objs.add(s.Sphere(*sp))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 0.0, 8.0), (0.0, 0.0, 0.0), 40.0, **frame)


def world_wide(rt, s, frame, n=900):
    """scripts/sphere_scaling.py's world of n + 4 spheres under the book-1 camera's view, 16 spp"""
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
    return _under_bvh(s, objs), None, _camera(rt, s, (13.0, 2.0, 3.0), (0.0, 0.0, 0.0), 20.0, **dict(frame, spp=16))


def _case(world, frame):
    return lambda rt, s: world(rt, s, frame)


WORLDS = {"sparse": _case(world_sparse, FULL), "nested": _case(world_nested, FULL),
          "lattice": _case(world_lattice, FULL), "mixed": _case(world_mixed, FULL),
          "mixed_bvh": _case(world_mixed_bvh, FULL), "wide": _case(world_wide, FULL),
          "sparse_thin": _case(world_sparse, THIN), "nested_thin": _case(world_nested, THIN),
          "lattice_thin": _case(world_lattice, THIN), "mixed_thin": _case(world_mixed, THIN),
          "listed": _case(world_listed, FULL), "listed_thin": _case(world_listed, THIN)}
# render flags of a world on the GPU (RT_FLAG_REFERENCE_BVH = 1: the reference's BVH topology, lists kept)
FLAGS = {"mixed": 1, "mixed_thin": 1}


def _render(api, rt, build, on_gpu, flags=0):
    scene = rt.Scene(api)
    world, lights, cam = build(scene)
    lin, _, st = cam.render(world, lights, seed=1, flags=flags)  # raises on a check failure (RT_EPANIC)
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
def test_walk_rounds_equal_the_oracle(builds, oracle_frames, rt, capi, name, build):
    api = builds[build]
    make = lambda s: WORLDS[name](rt, s)
    flags = FLAGS.get(name, 0)
    g, gpart, gst = _render(api, rt, make, True, flags)
    o, opart, ost = oracle_frames(name)
    assert g.shape == o.shape == ((4, 8, 3) if name.endswith("_thin") else (18, 32, 3))
    assert gst.panics == 0 and ost.panics == 0
    div = divergence(gpart, opart)
    rmse = rmse_per_channel(g, o)
    differing = int(np.any(g != o, axis=-1).sum())
    print(f"{name} / {build}: per-channel RMSE {rmse}, pixels differing from the oracle {differing}, "
          f"diverged (pixel, s_i) sums {div}")
    # every world runs the basic tier; "wide" its wide variant (more nodes than
    # the batch variant's LDS copy holds: RT_NODE_LDS_BATCH_BYTES / 112 = 365)
    s = rt.Scene(api)
    w, _, cam = make(s)
    info = capi.RtWorldInfo()
    assert api.world_info_get(s.s, w.h, -1, cam.background.h, flags, ctypes.byref(info)) == 0
    assert info.kernel_tier == 0
    assert (info.bvh_nodes > 365) == (name == "wide"), info.bvh_nodes
    if name.startswith("listed"):  # lists and spheres only
        assert info.bvh_nodes == 0
    if name.startswith("mixed") and flags:
        # the list is kept beside its BVH: its runs of refs and boxes are in the world's
        # blob, which the default flatten (one BVH over the elements) does not hold
        plain = capi.RtWorldInfo()
        assert api.world_info_get(s.s, w.h, -1, cam.background.h, 0, ctypes.byref(plain)) == 0
        assert info.bvh_nodes > 0 and info.device_bytes > plain.device_bytes, (info.device_bytes, plain.device_bytes)
    assert np.all(rmse == 0.0), rmse
    np.testing.assert_array_equal(g, o)
    assert div == 0
