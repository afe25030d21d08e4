"""OBJ materials as Disney BSDFs on the GPU (rt_wavefront_load_flags with
RT_OBJ_DISNEY): the first worlds in which kernel tier 5 runs F_DISNEY together
with remap_record (vertex normals, texture coordinates, a normal map),
image-ratio Mix and DiffuseLight around a Disney material.

  1. the reference's mc.obj from its own mc.mtl against the test-side
     restatement (tests/cpp/obj_disney_oracle.cpp), sky-lit and through the
     light mixture;
  2. scenes.obj_scene (small), disney_scene and background_scene likewise;
  3. rt_world_scatter on the frame's primary rays, every field bit-equal;
  4. the eight-key MTL mapping against a hand-built rt_mat_disney twin, without
     the oracle;
  5. the differential test of tests/test_obj_disney_cpu.py on the product.

Frames are 32 x 18, 16 spp, depth 10, seed 1; the bar of 1. and 2. is RMSE
exactly 0, no diverged (pixel, s_i) sum and equal panic counts.  Every test
here needs the new entry point or the new scene builders.
"""
import numpy as np
import pytest

from conftest import divergence
import obj_disney_query as oq
import radiance_query as rq
import scatter_query as sq
from test_parity_gpu import check, gpu_partials

pytestmark = pytest.mark.gpu

# (background_scene holds no Disney material and no BVH: the flat tier)
TIERS = {"mc": 5, "mc_lit": 5, "obj_scene": 5, "disney_scene": 5, "background_scene": 3}


def _render_parity(gpu, rt, name):
    s = rt.Scene(gpu)
    world, lights, cam = oq.WORLDS[name](s)
    info = oq.world_info(gpu, s, world, lights, cam.background)
    assert info.kernel_tier == TIERS[name]
    lin, srgb, st = cam.render(world, lights, seed=1)
    part = gpu_partials(gpu, s, cam, lin.shape[0])
    o_lin, o_srgb, o_part, o_panics = oq.reference(name)
    div = divergence(part, o_part)
    print(f"{name}: tier {info.kernel_tier}, features {info.features:#x}, panics gpu {st.panics} / oracle {o_panics}, "
          f"diverged {div}, max |partial difference| {np.abs(part - o_part).max():.3e}, sRGB bytes differing "
          f"{int((srgb != o_srgb).sum())}")
    rmse = check({"gpu": (lin, srgb, part), "oracle": (o_lin, o_srgb, o_part)}, max_div=0.0)
    assert np.all(rmse == 0.0), rmse
    assert div == 0.0
    assert srgb.tobytes() == o_srgb.tobytes()
    assert int(st.panics) == o_panics
    assert lin.max() > 0.05 and lin.std() > 0.01  # the frame shows something
    return info


# ---------------------------------------------------------------- 1. "mc" from its own MTL
@pytest.mark.parametrize("name", ["mc", "mc_lit"])
def test_mc_render_parity(gpu, rt, name):
    info = _render_parity(gpu, rt, name)
    want = oq.feature_bits("F_DISNEY", "F_REMAP")
    assert info.features & want == want
    if name == "mc_lit":  # the light shows: another frame than the sky-lit one
        assert oq.reference("mc_lit")[0].tobytes() != oq.reference("mc")[0].tobytes()


# ---------------------------------------------------------------- 2. main.rs's scenes
@pytest.mark.parametrize("name", ["obj_scene", "disney_scene", "background_scene"])
def test_scene_render_parity(gpu, rt, name):
    info = _render_parity(gpu, rt, name)
    if name == "obj_scene":
        want = oq.feature_bits("F_DISNEY", "F_PORTAL", "F_MEDIUM", "F_XFORM", "F_REMAP", "F_NORMALMAP")
        assert info.features & want == want, hex(info.features)


# ---------------------------------------------------------------- 3. one ray_color level on "mc"
def test_scatter_query_on_mc(gpu, rt):
    """rt_world_scatter on the frame's 576 primary rays with eval directions:
    every field of every record as orcx_world_scatter gives it (floats as
    integers; hit.mat, an index of the flattening, left out, as
    tests/test_world_scatter_gpu.py leaves it out).  No ray is left out."""
    drv = oq.driver()
    so = rt.Scene(drv)
    o_world, _, o_cam = oq.world_mc(so)
    rays = rq.camera_rays(drv, so, o_cam, seed=1)
    assert rays.shape == (oq.WIDTH * 18, 8)
    ev = np.random.default_rng(rq.RAY_SEED).standard_normal((len(rays), 3))
    ev /= np.linalg.norm(ev, axis=1)[:, None]
    s = rt.Scene(gpu)
    world, _, cam = oq.world_mc(s)
    for kw in (dict(vertex=1, sample=0), dict(vertex=3, sample=2)):
        want = sq.oracle_scatter(drv, so, o_world, rays, eval_dirs=ev, background=o_cam.background, **kw)
        got = s.scatter(world, None, rays, eval_dirs=ev, background=cam.background, seed=rq.SEED, **kw)
        bad = sq.differing_fields(got, want)
        f = want["flags"]
        print(f"mc {kw}: {len(want)} records; oracle: hits {int((want['hit']['flags'] & 1).sum())}, "
              f"RAY {int(((f & sq.RAY) != 0).sum())}, PDF {int(((f & sq.PDF) != 0).sum())}, "
              f"NO_SAMPLE {int(((f & sq.NO_SAMPLE) != 0).sum())}, PANIC {int(((f & sq.PANIC) != 0).sum())}, "
              f"emitting {int(want['emitted'].any(axis=1).sum())}, draws {np.bincount(want['draws']).tolist()}")
        if bad:
            sq.report(f"mc {kw}", got, want, bad)
        assert not bad, {k: len(v) for k, v in bad.items()}
        hit = (want["hit"]["flags"] & 1) != 0
        assert 100 <= hit.sum() <= len(rays) - 100
        assert ((f & sq.PDF) != 0).sum() >= 100  # Disney samples under remap_record
        assert want["emitted"][hit].any()          # map_Ke: DiffuseLight(image, Disney)


# ---------------------------------------------------------------- 4. the mapping against a hand-built twin
@pytest.mark.parametrize("ke", [oq.TWIN_KE, None], ids=["Ke", "no_Ke"])
def test_mtl_mapping_equals_a_hand_built_disney(gpu, rt, ke):
    """One triangle whose remap_record is the identity, its MTL setting all
    eight keys to distinct values over a solid Kd, against s.Triangle under
    s.Disney(SolidColor(Kd), the same values): 64 front-face rays, the same
    seed and indices, byte-equal records in every field a material decides."""
    rays, ev = oq.tri_rays(64)
    idx = (np.arange(64, dtype=np.uint32) * 7919) % 100003
    out = []
    for build in (oq.world_tri_loaded, oq.world_tri_twin):
        s = rt.Scene(gpu)
        world = build(s, ke)
        info = oq.world_info(gpu, s, world)
        assert info.kernel_tier == 5 and info.primitives == 1
        out.append(s.scatter(world, None, rays, eval_dirs=ev, indices=idx, seed=rq.SEED, vertex=2, sample=1))
    loaded, twin = out
    front = 3  # RT_HIT_FOUND | RT_HIT_FRONT_FACE
    assert np.all(loaded["hit"]["flags"] == front) and np.all(twin["hit"]["flags"] == front)
    assert np.all((loaded["flags"] & sq.PDF) != 0) and not (loaded["flags"] & sq.PANIC).any()
    for k in ("emitted", "f", "pdf", "origin", "dir", "eval_f", "eval_pdf", "flags", "draws"):
        assert sq.same_bytes(loaded[k], twin[k]), k
    sampled = (loaded["flags"] & sq.NO_SAMPLE) == 0
    assert sampled.sum() >= 48 and loaded["pdf"][sampled].min() > 0 and loaded["f"].max() > 0
    assert loaded["emitted"].any() == (ke is not None)
    # the loaded values matter: the default parameter set gives other records
    s = rt.Scene(gpu)
    tris = s.Hittables()
    tris.add(s.Triangle(oq.TRI_A, oq.TRI_U, oq.TRI_V, s.Disney(s.SolidColor(oq.TWIN_KD))))
    plain = s.scatter(tris, None, rays, eval_dirs=ev, indices=idx, seed=rq.SEED, vertex=2, sample=1)
    assert not sq.same_bytes(plain["f"], loaded["f"])


# ---------------------------------------------------------------- 5. the differential test on the product
def test_eight_key_mapping_differential_on_the_gpu(gpu):
    moved = oq.differential(gpu)
    assert sorted(moved) == sorted(["Pr", "aniso", "Ps", "Pm", "Pc", "Pcr", "Ni", "Tf"])
    assert all(moved.values()), moved
