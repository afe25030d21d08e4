"""The work queue's hand-out on the GPU against the oracle.  Every tier's loop
of rt_path_kernel (raytracer-2025_amd/csrc/rt_kernel_path.hip) takes its queue
entries through one refill (rt_queue.h): the wave's pool of entries lives in
scalar registers, a chunk is sized only on the pass that takes one from the
counter, and a pass that lies in one region of the queue (whole rows, parts,
fine parts) decodes its entries with that region's constants.  None of that
may move a sample: the f32 frames equal the oracle's bit for bit, no (pixel,
stratum row) sum diverges and the render reports no error -- on the product
and on the check build.

Basic tier (test_walk_rounds_gpu's four far-apart spheres, a mirror ball in
glass among them), frames chosen by their queue:

    4x2   at 1 spp    8 entries: fewer than one wave's lanes
    8x8   at 1 spp    64: exactly a wave's first pool
    13x5  at 1 spp    65: one entry from the counter
    16x9  at 4 spp    288 whole rows of two samples (a row that short has no parts)
    16x9  at 25 spp   720 rows of five samples: whole rows, 2 parts a row on
                      the frame's last five image rows, 5 parts on its last
    16x9  at 25 spp   as three shards, rows k, k + 3, k + 6 (k = 0, 1, 2): each
                      shard's queue ends on its own tail rows

and one frame each on the smallest world of the mesh tier (a quad beside a
sphere, 16x9 at 25 spp: its parts are two samples) and of the flat full tier
(the Cornell box with its smoke, 12x12 at 9 spp), whose loop shares the
refill."""
import ctypes
import os

import numpy as np
import pytest

from conftest import divergence
from test_parity_gpu import gpu_partials
from test_walk_rounds_gpu import world_sparse

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")


def _sparse(width, height, spp):
    return lambda rt, scenes, s: world_sparse(rt, s, {"width": width, "aspect": width / height, "spp": spp})


def _quad_and_sphere(rt, scenes, s):
    red = s.Lambertian(s.SolidColor((0.8, 0.3, 0.2)))
    objs = s.Hittables()
    objs.add(s.Quad((-2.0, -1.0, -1.0), (4.0, 0.0, 0.0), (0.0, 0.0, 3.0), s.Lambertian(s.SolidColor((0.2, 0.5, 0.7)))))
    objs.add(s.Sphere((0.0, 0.0, 0.0), 1.0, s.Dielectric(s.SolidColor((1.0, 1.0, 1.0)), 1.5)))
    objs.add(s.Sphere((1.5, -0.5, 1.0), 0.5, red))
    w = s.Hittables()
    w.add(s.BVH(objs))
    cam = rt.Camera()
    cam.aspect_ratio = 16 / 9
    cam.image_width = 16
    cam.samples_per_pixel = 25
    cam.max_depth = 8
    cam.vertical_fov_in_degrees = 40.0
    cam.look_from = (0.0, 2.0, 8.0)
    cam.look_at = (0.0, 0.0, 0.0)
    cam.vec_up = (0.0, 1.0, 0.0)
    cam.background = s.SkyGradient()
    return w, None, cam


def _cornell(rt, scenes, s):
    return scenes.cornell_smoke(s, 12, 9)


# name: (world, (height, width), tier, [(row_offset, row_stride)])
CASES = {
    "4x2_s1": (_sparse(4, 2, 1), (2, 4), 0, [(0, 1)]),
    "8x8_s1": (_sparse(8, 8, 1), (8, 8), 0, [(0, 1)]),
    "13x5_s1": (_sparse(13, 5, 1), (5, 13), 0, [(0, 1)]),
    "16x9_s4": (_sparse(16, 9, 4), (9, 16), 0, [(0, 1)]),
    "16x9_s25": (_sparse(16, 9, 25), (9, 16), 0, [(0, 1)]),
    "16x9_s25_shards": (_sparse(16, 9, 25), (9, 16), 0, [(0, 3), (1, 3), (2, 3)]),
    "mesh_16x9_s25": (_quad_and_sphere, (9, 16), 1, [(0, 1)]),
    "flat_12x12_s9": (_cornell, (12, 12), 3, [(0, 1)]),
}


def _render(api, rt, scenes, name, on_gpu):
    """[(linear f32 rows, f64 (pixel, s_i) sums, stats)] of the case's shards"""
    build, _, _, shards = CASES[name]
    scene = rt.Scene(api)
    world, lights, cam = build(rt, scenes, scene)
    out = []
    for off, stride in shards:
        lin, _, st = cam.render(world, lights, seed=1, row_offset=off, row_stride=stride)  # raises on a check failure
        if on_gpu:
            part = gpu_partials(api, scene, cam, lin.shape[0])
        else:
            part, _ = cam.render_partials(world, lights, seed=1, row_offset=off, row_stride=stride)
        out.append((lin, part, st))
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
def test_refill_equals_the_oracle(builds, oracle_frames, rt, scenes, capi, name, build):
    api = builds[build]
    make, (height, width), tier, shards = CASES[name]
    s = rt.Scene(api)
    w, lights, cam = make(rt, scenes, s)
    assert (cam.image_height, cam.image_width) == (height, width)
    info = capi.RtWorldInfo()
    assert api.world_info_get(s.s, w.h, -1 if lights is None else lights.h, cam.background.h if cam.background else -1,
                              0, ctypes.byref(info)) == 0
    assert info.kernel_tier == tier
    got = _render(api, rt, scenes, name, True)
    want = oracle_frames(name)
    rows = 0
    for (off, stride), (g, gpart, gst), (o, opart, ost) in zip(shards, got, want):
        assert g.shape == o.shape == (len(range(off, height, stride)), width, 3)
        assert gst.panics == 0 and ost.panics == 0
        assert gst.samples == g.shape[0] * width * cam.sqrt_spp ** 2
        div = divergence(gpart, opart)
        differing = int(np.any(g != o, axis=-1).sum())
        print(f"{name} / {build} rows {off}::{stride}: pixels differing from the oracle {differing}, "
              f"diverged (pixel, s_i) sums {div}")
        np.testing.assert_array_equal(g, o)
        assert div == 0
        rows += g.shape[0]
    assert rows == height
