"""The basic tier's boxed sphere children against the oracle: a sphere child of
a 4-wide node carries its own f32 box, the walk slab-tests it and queues the
sphere for the exact f64 Sphere::hit on a box hit (rt_walk4.h visit4_rows,
rth::bvh4_convert).  A box admits more rays than the sphere does, so these
small worlds load the per-lane queue and the boxes' edge cases; none of it may
change a sample: the f32 frames are equal to the oracle's and no (pixel,
stratum row) sum diverges.  Frames of at most 64x48 pixels, 16 spp, depth 12.

(a) twelve overlapping and nested spheres along the view axis under one BVH:
    a central ray pierces more boxes than a lane's queue holds (RT_PEND_CAP =
    8), so lanes wait for a sphere round with a full queue;
(b) the camera inside a Dielectric sphere that is a BVH child;
(c) a lattice of r = 0.5 spheres at integer centres -- c +- r exact in f32, no
    rounding slack in the boxes -- seen from an integer point along -z through
    an odd-sized frame, whose centre column looks along the lattice planes.
    The samples are jittered inside their pixels, so hardly any ray here has a
    direction component of exactly zero, and no camera can give every sample
    one (the viewport would have to lie in a plane through the eye): the +-0 /
    clamped 1/d path through a zero-slack box is held by the CPU property
    test (tests/test_sphere_box_cpu.py), and on the device by
    tests/test_walk_filters_gpu.py for slab_f itself; this world holds the
    near-zero components and the exactly representable boxes;
(d) world (a) translated by (4096, 0, 4096), with radii from 1e-3 to 1000 (a
    ground sphere under the string, a sphere of r = 40 behind it);
(e) about 800 spheres: a tree of more than 365 nodes, which the basic tier's
    wide variant (rt_path_kernel<0, true>) runs.
"""
import ctypes

import numpy as np
import pytest

from conftest import divergence
from test_parity_gpu import render_both

pytestmark = pytest.mark.gpu


def _camera(rt, s, look_from, look_at, width=64, aspect=4 / 3, fov=40.0, depth=12, spp=16):
    cam = rt.Camera()
    cam.aspect_ratio = aspect
    cam.image_width = width
    cam.samples_per_pixel = spp
    cam.max_depth = depth
    cam.vertical_fov_in_degrees = fov
    cam.look_from = look_from
    cam.look_at = look_at
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.background = s.SkyGradient()
    return cam


def _mats(s):
    return [s.Lambertian(s.SolidColor((0.8, 0.3, 0.2))), s.Dielectric(s.SolidColor((1.0, 1.0, 1.0)), 1.5),
            s.Lambertian(s.SolidColor((0.2, 0.5, 0.7)))]


def _under_bvh(s, objs):
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w


def world_axis(rt, s, off=(0.0, 0.0, 0.0), radii=None, extra=()):
    """Twelve spheres strung along the view axis (z), each overlapping the next,
    every third one nested in its neighbour."""
    mats = _mats(s)
    objs = s.Hittables()
    ox, oy, oz = off
    for i in range(12):
        nested = i % 3 == 2  # almost concentric with sphere i - 1, inside it
        z = -5.5 + (i - 1 + 0.1 if nested else i)
        r = radii[i] if radii else (0.3 if nested else 0.7)
        objs.add(s.Sphere((ox + 0.05 * (i % 2), oy, oz + z), r, mats[i % 3]))
    for k, (c, r) in enumerate(extra):
        objs.add(s.Sphere((ox + c[0], oy + c[1], oz + c[2]), r, mats[(k + 2) % 3]))
    cam = _camera(rt, s, (ox, oy + 0.1, oz + 9.0), (ox, oy, oz), fov=25.0)
    return _under_bvh(s, objs), None, cam


def world_inside(rt, s):
    mats = _mats(s)
    objs = s.Hittables()
    objs.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, mats[2]))
    objs.add(s.Sphere((0.0, 1.0, 6.0), 3.0, mats[1]))  # the camera is at its centre
    for i in range(6):
        objs.add(s.Sphere((-2.5 + i, 0.4, 0.5 * (i % 2)), 0.4, mats[i % 3]))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 1.0, 6.0), (0.0, 0.3, 0.0))


def world_lattice(rt, s):
    mats = _mats(s)
    objs = s.Hittables()
    k = 0
    for x in (-2, -1, 0, 1, 2):
        for y in (-1, 0, 1):
            for z in (-3, -2, -1, 0):
                objs.add(s.Sphere((float(x), float(y), float(z)), 0.5, mats[k % 3]))
                k += 1
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 0.0, 5.0), (0.0, 0.0, 0.0), width=63, aspect=63 / 47)


def world_offset(rt, s):
    radii = [0.7, 0.7, 1e-3, 0.7, 0.7, 0.01, 0.7, 0.7, 0.3, 0.7, 0.7, 0.05]
    extra = [((0.0, -1000.75, 0.0), 1000.0), ((0.0, 30.0, -70.0), 40.0), ((0.3, 0.2, 6.0), 1e-3)]
    return world_axis(rt, s, off=(4096.0, 0.0, 4096.0), radii=radii, extra=extra)


def world_many(rt, s, n=800):
    import random
    rnd = random.Random(n)
    mats = _mats(s)
    objs = s.Hittables()
    objs.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, mats[2]))
    for i in range(n):
        objs.add(s.Sphere((rnd.uniform(-4, 4), 0.1, rnd.uniform(-6, 3)), 0.1, mats[i % 3]))
    return _under_bvh(s, objs), None, _camera(rt, s, (0.0, 1.0, 6.0), (0.0, 0.3, 0.0))


WORLDS = {"axis": world_axis, "inside": world_inside, "lattice": world_lattice, "offset": world_offset,
          "many": world_many}


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_boxed_sphere_worlds_equal_the_oracle(gpu, oracle, rt, capi, name):
    build = lambda s: WORLDS[name](rt, s)
    out, st = render_both(gpu, oracle, rt, build)
    g, o = out["gpu"], out["oracle"]
    assert g[0].shape == o[0].shape and g[0].shape[0] <= 48 and g[0].shape[1] <= 64
    assert st["gpu"].panics == 0 and st["oracle"].panics == 0
    div = divergence(g[2], o[2])
    differing = int(np.any(g[0] != o[0], axis=-1).sum())
    print(f"{name}: pixels differing from the oracle {differing}, diverged (pixel, s_i) sums {div}")
    # every world runs the basic tier; "many" its wide variant (more nodes than
    # the batch variant's LDS copy holds: RT_NODE_LDS_BATCH_BYTES / 112 = 365)
    s = rt.Scene(gpu)
    w, _, cam = build(s)
    info = capi.RtWorldInfo()
    assert gpu.world_info_get(s.s, w.h, -1, cam.background.h, 0, ctypes.byref(info)) == 0
    assert info.kernel_tier == 0
    assert (info.bvh_nodes > 365) == (name == "many"), info.bvh_nodes
    np.testing.assert_array_equal(g[0], o[0])
    assert div == 0
