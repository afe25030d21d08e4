"""The worlds of tests/test_walk_rounds_gpu.py on the oracle alone: none is
degenerate.  The oracle's work counters (oracle/rt_oracle.hpp WorkCounts) of
each frame must show what the GPU test relies on:

* sphere hits (`emitted`: one per hit) and sky misses;
* glass scatters (`dielectric`);
* paths cut at the depth limit: every material of these worlds (Lambertian,
  Metal without fuzz, Dielectric) scatters at every hit, so a path ends in a
  sky miss or at max_depth, and the cut paths are camera_rays - sky_miss;
* in the nested world every hit is a glass scatter (the nine outer shells
  hide the opaque core from these paths), so its cut paths are glass paths,
  and they are a tenth of all paths and more: the ones into the shells at
  the frame's centre, which meet more spheres than a lane's queue holds
  (RT_PEND_CAP = 8).

What the counters cannot show is which material a cut path met: they are
totals of a frame.  In the other full frames the cut paths are asked for as
such, beside the glass scatters; the sparse world is built so that glass is
where paths stay (a mirror ball inside a sphere of index 2.4, total
reflection past 25 degrees), and its other spheres are too far apart to hold
a path for eight bounces.

The thin frames (8x4 pixels, 1 spp) hold 32 paths.  They must show hits,
misses and glass scatters.  Cut paths are 0.1 - 1 % of the full frames' paths
outside the nested world (2 ... 26 of 2304), so a 32-path frame of those
worlds expects less than one and is not asked for any; the nested thin
frame, whose central pixels look into the shells, is.
"""
import ctypes

import pytest

from test_walk_rounds_gpu import WORLDS

FIELDS = ["camera_rays", "ray_color_calls", "bvh_node_tests", "sphere_tests", "sphere_disc_ok", "sphere_records",
          "quad_tests", "tri_tests", "planar_records", "lambert", "metal", "dielectric", "isotropic", "sky_miss",
          "medium_tests", "light_pdf", "transform_tests", "emitted"]


def _counts(oracle, rt, name):
    assert oracle.work_count_fields() == len(FIELDS)
    scene = rt.Scene(oracle)
    world, lights, cam = WORLDS[name](rt, scene)
    c = cam.to_c()
    opts = rt.Camera._opts(oracle, 1, 0, 1, 0, 0)[0]
    wc = (ctypes.c_uint64 * len(FIELDS))()
    oracle.check(oracle.render_f64(scene.s, world.h, -1 if lights is None else lights.h, ctypes.byref(c),
                                   ctypes.byref(opts), None, None, None, wc))
    return dict(zip(FIELDS, wc)), cam


@pytest.mark.parametrize("name", sorted(WORLDS))
def test_world_has_hits_misses_and_cut_glass_paths(oracle, rt, name):
    n, cam = _counts(oracle, rt, name)
    thin = name.endswith("_thin")
    rows = 4 if thin else 18
    assert n["camera_rays"] == rows * cam.image_width * cam.sqrt_spp ** 2
    cut = n["camera_rays"] - n["sky_miss"]
    print(f"{name}: {n['camera_rays']} paths, {n['emitted']} hits, {n['sky_miss']} misses, {n['dielectric']} glass "
          f"scatters, {cut} paths cut at depth {cam.max_depth}, {n['sphere_tests'] / n['ray_color_calls']:.2f} "
          f"sphere tests a ray")
    # every hit scattered: nothing but a miss or the depth limit ends a path
    assert n["lambert"] + n["metal"] + n["dielectric"] == n["emitted"]
    assert n["ray_color_calls"] == n["emitted"] + n["sky_miss"]
    assert n["emitted"] > 0 and n["sky_miss"] > 0
    assert n["dielectric"] > 0
    if not thin or name == "nested_thin":
        assert cut > 0
    if name.startswith("nested"):
        # a path into the nine glass shells scatters at each: the paths through the
        # frame's centre are cut before they are out again, a tenth of all and more
        assert 10 * cut >= n["camera_rays"]
        assert n["dielectric"] == n["emitted"]  # ... and every one of them a glass path
