"""The Portal material on the GPU (the M_PORTAL arm of shade() in kernel tiers 4
and 5) against the test-side restatement (tests/cpp/portal_oracle.cpp): three
rendered worlds, each at RMSE 0 with no diverged (pixel, s_i) sum, equal sRGB
bytes and equal panic counts; and the hit / occlusion queries of a Portal
world, which flatten it without F_PORTAL.

Every test here needs rt_mat_portal, so none passes without the material.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import divergence
import portal_query as pq
from test_parity_gpu import check, gpu_partials

pytestmark = pytest.mark.gpu


def _info(gpu, capi, s, world, lights, cam):
    info = capi.RtWorldInfo()
    bg = cam.background.h if cam.background is not None else -1
    gpu.check(gpu.world_info_get(s.s, world.h, -1 if lights is None else lights.h, bg, 0, C.byref(info)))
    return info


@pytest.mark.parametrize("name", list(pq.WORLDS))
def test_render_parity(gpu, rt, capi, name):
    """32 x 18, 16 spp, depth 10, seed 1: the kernel tier as stated, per-channel
    RMSE exactly 0, no diverged (pixel, s_i) sum, the sRGB bytes (world 1: the
    ACES tone map) equal, the same panic count on both sides."""
    s = rt.Scene(gpu)
    world, lights, cam = pq.WORLDS[name](s)
    info = _info(gpu, capi, s, world, lights, cam)
    assert info.kernel_tier == pq.TIERS[name] and info.features & pq.feature_bit("F_PORTAL")
    lin, srgb, st = cam.render(world, lights, seed=1)
    part = gpu_partials(gpu, s, cam, lin.shape[0])
    o_lin, o_srgb, o_part, o_panics = pq.reference(name)
    div = divergence(part, o_part)
    print(f"{name}: tier {info.kernel_tier}, panics gpu {st.panics} / oracle {o_panics}, diverged {div}, "
          f"max |partial difference| {np.abs(part - o_part).max():.3e}, sRGB bytes differing "
          f"{int((srgb != o_srgb).sum())}")
    rmse = check({"gpu": (lin, srgb, part), "oracle": (o_lin, o_srgb, o_part)}, max_div=0.0)
    assert np.all(rmse == 0.0), rmse
    assert div == 0.0
    assert srgb.tobytes() == o_srgb.tobytes()
    assert int(st.panics) == o_panics
    assert lin.max() > 0.05  # the frame shows something
    # ... and the portals in it: the frame is not its Transparent twin's
    assert lin.tobytes() != pq.reference(name, portal=False)[0].tobytes()


def test_queries_see_the_portal_and_skip_its_tier(gpu, rt):
    """rt_world_hit on the `scene` world's 576 primary rays names the Portal's
    handle in `mat` where the quad is hit, and rt_world_occluded agrees with
    its FOUND flags.  Queries never shade, so they flatten the world without
    F_PORTAL: record for record and byte for byte what the Transparent twin
    returns (the same handles in the same order, the twin's tier), before and
    after a render has uploaded the world for tier 4."""
    import hit_query as hq
    recs, occ = [], []
    for portal in (True, False):
        s = rt.Scene(gpu)
        world, _, cam = pq.world_scene(s, portal=portal)
        saved = (hq.GRID_W, hq.GRID_H)
        hq.GRID_W, hq.GRID_H = 32, 18
        try:
            rays = hq.grid_rays(cam)
        finally:
            hq.GRID_W, hq.GRID_H = saved
        assert len(rays) == 576
        recs.append(s.hit(world, rays))
        occ.append(s.occluded(world, rays))
        if portal:  # a render in between: the query's world and the render's are flattened apart
            lin, _, st = cam.render(world, None, seed=1)
            assert st.panics == 0
            recs.append(s.hit(world, rays))
            occ.append(s.occluded(world, rays))
    found = (recs[0]["flags"] & 1) != 0
    # scenes.portal_scene makes the quad's material first: handle 0; the sphere's Lambertian is 1
    assert set(recs[0]["mat"][found]) == {0, 1}
    on_quad = found & (recs[0]["mat"] == 0)
    assert on_quad.sum() > 50 and np.abs(recs[0]["p"][on_quad][:, 1]).max() < 1e-9  # the y = 0 plane
    assert occ[0].tobytes() == found.astype(np.uint8).tobytes()
    for r in recs[1:]:
        assert r.tobytes() == recs[0].tobytes()
    for o in occ[1:]:
        assert o.tobytes() == occ[0].tobytes()
