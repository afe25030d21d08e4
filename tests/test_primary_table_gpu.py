"""The basic tier's primary rays from the per-pixel candidate table, against the
oracle.  The batch variant of rt_path_kernel<0> (rt_kernel_path.hip) resolves
a new sample's camera ray in the post-walk pass: the exact f64 sphere test on
the spheres the launch's table names for the pixel (rt_primary.h beam_may_hit,
rt_kernel_common.hip rt_primary_kernel), not a walk of the tree; a pixel with
more than eight candidates sends its rays through the walk.  None of that may
move a sample: on every world the f32 frame equals the oracle's bit for bit,
no (pixel, stratum row) sum diverges, RtStats.rays is the oracle's count and
no path panics -- on the product and on the check build, which also walks
every primary ray taken from the table and fails the render where the walk
finds another hit.  Frames of 64x36 or 48x48 pixels (the queue-shape frames of
tests/test_refill_gpu.py smaller still) at 16 spp or fewer.

    c2            C2's spheres and camera (lens radius 0.052)
    c2_pinhole    ... with defocus angle 0
    c2_lens10     ... with defocus angle 10 degrees (lens radius 0.87)
    c2_shards     ... as three row shards, rows k, k + 3, ... (k = 0, 1, 2)
    stack         twelve overlapping spheres along the view axis: the centre
                  pixels have more candidates than the table holds, the rim has
                  few -- table pixels and walked pixels share waves
    inside        the camera at the centre of a glass sphere
    sky           one sphere behind the camera: every primary ray misses
    touching      two spheres that touch on the centre ray of pixel (24, 24)
    list          spheres in a plain list, no BVH
    q65, q288     13x5 at 1 spp and 16x9 at 4 spp: queues that end in
                  1-sample entries
    wide          900 spheres: the wide variant, which builds no table
"""
import ctypes
import os

import numpy as np
import pytest

from conftest import divergence
from test_boxed_spheres_gpu import world_axis, world_inside, world_many
from test_parity_gpu import gpu_partials
from test_walk_rounds_gpu import world_sparse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")
CAP, NONE, WALK = 8, 0xFFFE, 0xFFFF


def _c2(defocus=None):
    def build(rt, scenes, s):
        w, lights, cam = scenes.random_spheres(s, 64, 16)
        if defocus is not None:
            cam.defocus_angle_in_degrees = defocus
        return w, lights, cam
    return build


def _camera(rt, s, look_from, look_at, width, aspect, fov=40.0, spp=16):
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
            s.Metal((0.7, 0.6, 0.5), 0.1)]


def _stack(rt, scenes, s):
    w, lights, cam = world_axis(rt, s)
    cam.aspect_ratio, cam.image_width, cam.max_depth = 16 / 9, 64, 8
    return w, lights, cam


def _inside(rt, scenes, s):
    w, lights, cam = world_inside(rt, s)
    cam.aspect_ratio, cam.image_width, cam.max_depth = 16 / 9, 64, 8
    return w, lights, cam


def _sky(rt, scenes, s):
    objs = s.Hittables()
    objs.add(s.Sphere((0.0, 0.0, 20.0), 2.0, _mats(s)[0]))
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w, None, _camera(rt, s, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), 64, 16 / 9)


def _touching(rt, scenes, s):
    # Camera::initilize (camera.rs:204-245) for this camera: from (0, 0, 9) down -z, focus distance 10,
    # 48x48 at fov 40; the centre of pixel (24, 24) lies half a pixel right of and below the axis
    h = np.tan(np.radians(40.0) / 2.0)
    px = 2.0 * h * 10.0 / 48.0
    d = np.array([0.5 * px, -0.5 * px, -10.0])
    t = np.array([0.0, 0.0, 9.0]) + 0.9 * d  # the touching point, on that pixel's centre ray
    mats = _mats(s)
    objs = s.Hittables()
    objs.add(s.Sphere(tuple(t - np.array([1.0, 0.0, 0.0])), 1.0, mats[0]))
    objs.add(s.Sphere(tuple(t + np.array([1.0, 0.0, 0.0])), 1.0, mats[2]))
    objs.add(s.Sphere(tuple(t + np.array([0.0, 2.0, 0.0])), 1.0, mats[1]))
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w, None, _camera(rt, s, (0.0, 0.0, 9.0), (0.0, 0.0, 0.0), 48, 1.0)


def _list(rt, scenes, s):
    mats = _mats(s)
    w = s.Hittables()
    w.add(s.Sphere((0.0, -100.5, 0.0), 100.0, mats[0]))
    for i in range(7):
        w.add(s.Sphere((-3.0 + i, 0.1 * (i % 3), -0.7 * (i % 2)), 0.5, mats[i % 3]))
    cam = _camera(rt, s, (0.0, 1.0, 7.0), (0.0, 0.0, 0.0), 64, 16 / 9)
    cam.defocus_angle_in_degrees = 1.0
    cam.focus_distance = 7.0
    return w, None, cam


def _sparse(width, height, spp):
    return lambda rt, scenes, s: world_sparse(rt, s, {"width": width, "aspect": width / height, "spp": spp})


def _wide(rt, scenes, s):
    w, lights, cam = world_many(rt, s, n=900)
    cam.aspect_ratio, cam.image_width, cam.max_depth = 16 / 9, 64, 8
    return w, lights, cam


WHOLE = [(0, 1)]
# name: (world, (height, width), [(row_offset, row_stride)])
CASES = {
    "c2": (_c2(), (36, 64), WHOLE),
    "c2_pinhole": (_c2(0.0), (36, 64), WHOLE),
    "c2_lens10": (_c2(10.0), (36, 64), WHOLE),
    "c2_shards": (_c2(), (36, 64), [(0, 3), (1, 3), (2, 3)]),
    "stack": (_stack, (36, 64), WHOLE),
    "inside": (_inside, (36, 64), WHOLE),
    "sky": (_sky, (36, 64), WHOLE),
    "touching": (_touching, (48, 48), WHOLE),
    "list": (_list, (36, 64), WHOLE),
    "q65": (_sparse(13, 5, 1), (5, 13), WHOLE),
    "q288": (_sparse(16, 9, 4), (9, 16), WHOLE),
    "wide": (_wide, (36, 64), WHOLE),
}


def _table(api, scene, rows, width):
    """The last render's candidate table [rows][width][8], or None where the kernel builds none."""
    tab = np.zeros((rows, width, CAP), dtype=np.uint16)
    rc = api.render_primary_get(scene.s, tab.ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)), tab.size)
    if rc == -6:  # RT_EUNSUPPORTED
        return None
    api.check(rc)
    return tab


def _render(api, rt, scenes, name, on_gpu):
    """[(linear f32 rows, f64 (pixel, s_i) sums, stats, candidate table)] of the case's shards"""
    build, _, shards = CASES[name]
    scene = rt.Scene(api)
    world, lights, cam = build(rt, scenes, scene)
    out = []
    for off, stride in shards:
        lin, _, st = cam.render(world, lights, seed=1, row_offset=off, row_stride=stride)  # raises on a check failure
        if on_gpu:
            part = gpu_partials(api, scene, cam, lin.shape[0])
            tab = _table(api, scene, lin.shape[0], cam.image_width)
        else:
            part, _ = cam.render_partials(world, lights, seed=1, row_offset=off, row_stride=stride)
            tab = None
        out.append((lin, part, st, tab))
    return out


@pytest.fixture(scope="module")
def oracle_frames(oracle, rt, scenes):
    """Each case's oracle frames, rendered once for both builds."""
    frames = {}

    def get(name):
        if name not in frames:
            frames[name] = _render(oracle, rt, scenes, name, False)
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
@pytest.mark.parametrize("name", sorted(CASES))
def test_primary_table_equals_the_oracle(builds, oracle_frames, rt, scenes, capi, name, build):
    api = builds[build]
    make, (height, width), shards = CASES[name]
    s = rt.Scene(api)
    w, lights, cam = make(rt, scenes, s)
    assert (cam.image_height, cam.image_width) == (height, width) and cam.samples_per_pixel <= 16
    info = capi.RtWorldInfo()
    assert api.world_info_get(s.s, w.h, -1, cam.background.h, 0, ctypes.byref(info)) == 0
    assert info.kernel_tier == 0
    # the batch variant's LDS copy holds 365 nodes (RT_NODE_LDS_BATCH_BYTES / 112); "wide" has more
    assert (info.bvh_nodes > 365) == (name == "wide"), info.bvh_nodes
    got = _render(api, rt, scenes, name, True)
    want = oracle_frames(name)
    rows = 0
    walked = tabled = 0
    for (off, stride), (g, gpart, gst, tab), (o, opart, ost, _) in zip(shards, got, want):
        assert g.shape == o.shape == (len(range(off, height, stride)), width, 3)
        assert gst.panics == 0 and ost.panics == 0
        div = divergence(gpart, opart)
        differing = int(np.any(g != o, axis=-1).sum())
        print(f"{name} / {build} rows {off}::{stride}: pixels differing from the oracle {differing}, diverged "
              f"(pixel, s_i) sums {div}, rays {gst.rays} (oracle {ost.rays})")
        np.testing.assert_array_equal(g, o)
        assert div == 0
        assert gst.rays == ost.rays
        if name == "wide":
            assert tab is None  # the wide variant builds no table
        else:
            assert tab is not None
            walk = tab[:, :, 0] == WALK
            n = (tab < NONE).sum(axis=-1)
            print(f"  candidates a pixel: mean {n[~walk].mean() if (~walk).any() else 0:.2f}, most {n.max()}, "
                  f"walked pixels {int(walk.sum())} of {walk.size}")
            walked += int(walk.sum())
            tabled += int((~walk).sum())
            # a row's candidates are ascending sphere indices, the unused slots behind them
            v = tab[~walk].astype(np.int64)
            assert np.all((v[:, 1:] > v[:, :-1]) | (v[:, 1:] == NONE))
            assert np.all(v[v < NONE] < info.primitives)
            if name == "sky":
                assert not walk.any() and n.max() == 0
        rows += g.shape[0]
    assert rows == height
    if name == "stack":
        assert walked > 0 and tabled > 0, (walked, tabled)
