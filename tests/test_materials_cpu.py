"""The wrapper and pass-through materials and the Perlin tables past the first,
without a device: which kernel tier and feature bits each world of
tests/material_worlds.py gets (rt_world_info_get flattens a world as a render
does), what the builders refuse, and the oracle on its own -- the furnace and
emission worlds hold it to closed-form answers, and every world of
tests/test_materials_gpu.py renders on it without a panic, so a parity test
there never passes by both sides panicking."""
import ctypes

import numpy as np
import pytest

import material_worlds as mw
from test_tiers_cpu import info_of

RT_EHANDLE, RT_EUNSUPPORTED = -2, -6


@pytest.mark.parametrize("name", mw.ALL)
def test_tier_and_features(product, capi, rt, name):
    """The flat full tier (3) for a list, the BVH full tier (2) under a BVH,
    FULL_GL (4) for wrapper trees deeper than one level and Mix::from_image;
    F_MATFULL for every wrapper, F_TEXFULL only where an image or a noise
    texture is in use, F_GENERAL only with tier 4."""
    s = rt.Scene(product)
    world, lights, cam = mw.build(rt, s, name)
    info = info_of(product, capi, s, world, lights, cam.background)
    tier, features = mw.expected(name)
    assert info.kernel_tier == tier
    assert info.features & mw.F_MASK == features
    assert (info.bvh_nodes > 0) == (name in mw.CASES and mw.CASES[name].objects == "bvh")


def _sphere_bvh(s):
    mat = s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))
    objs = s.Hittables()
    for i in range(5):
        objs.add(s.Sphere((float(i), 0.0, 0.0), 0.25, mat))
    w = s.Hittables()
    w.add(s.BVH(objs))
    return w, mat


@pytest.mark.parametrize("unused", ["mix", "mix_image", "nested_mix", "too_deep_mix", "transparent", "isotropic", "noise",
                                    "light_of_light"])
def test_unused_materials_keep_the_tier(product, capi, rt, unused):
    """Materials and textures no emitted primitive reaches decide nothing: a
    sphere BVH stays on the basic tier with no full-tier feature, whatever
    else the scene holds (a Mix chain past the depth limit included)."""
    s = rt.Scene(product)
    w, mat = _sphere_bvh(s)
    if unused == "mix":
        s.Mix(mat, s.Metal((0.8, 0.8, 0.8), 0.0), 0.5)
    elif unused == "mix_image":
        s.Mix_from_image(mat, s.Transparent(), s.ImageTexture(mw.alpha_image()))
    elif unused == "nested_mix":
        mw.nested_mix(s, 3)
    elif unused == "too_deep_mix":
        mw.nested_mix(s, 5)
    elif unused == "transparent":
        s.Transparent()
    elif unused == "isotropic":
        s.Isotropic(s.SolidColor((1, 1, 1)))
    elif unused == "noise":
        s.Lambertian(s.NoiseTexture(0.3, 5))
    else:
        s.DiffuseLight(s.SolidColor((1, 1, 1)), s.DiffuseLight(s.SolidColor((1, 1, 1))))
    info = info_of(product, capi, s, w, None, s.SkyGradient())
    assert info.kernel_tier == 0
    assert info.features & mw.F_MASK == 0


def test_unused_wrappers_do_not_make_a_full_world_general(product, capi, rt):
    """A world of the flat full tier stays there beside an unused nested Mix,
    an unused Mix::from_image and an unused NoiseTexture."""
    s = rt.Scene(product)
    mw.nested_mix(s, 4)
    s.Mix_from_image(s.Transparent(), s.EmptyMaterial(), s.ImageTexture(mw.alpha_image()))
    s.Lambertian(s.NoiseTexture(0.3, 5))
    world, lights, cam = mw.build(rt, s, "const_flat_lit")
    info = info_of(product, capi, s, world, lights, cam.background)
    assert info.kernel_tier == 3
    assert info.features & mw.F_MASK == mw.F["F_MATFULL"]


def _world_of(s, mat):
    w = s.Hittables()
    w.add(s.Sphere((0, 0, -2), 1.0, mat))
    return w


def test_wrapper_depth_limit(product, capi, rt):
    """Four nested Mix levels are a tier-4 world; five are refused with the
    message that names the limit."""
    s = rt.Scene(product)
    info = info_of(product, capi, s, _world_of(s, mw.nested_mix(s, 4)))
    assert info.kernel_tier == 4
    s = rt.Scene(product)
    w = _world_of(s, mw.nested_mix(s, 5))
    rc = product.world_info_get(s.s, w.h, -1, -1, 0, ctypes.byref(capi.RtWorldInfo()))
    assert rc == RT_EUNSUPPORTED
    assert b"4 levels" in product.last_error()


def test_bad_handles(product, rt):
    s = rt.Scene(product)
    ok = s.EmptyMaterial().h
    solid = s.SolidColor((1, 1, 1)).h
    noise = s.NoiseTexture(1.0, 1).h
    image = s.ImageTexture(mw.alpha_image()).h
    for bad in (-1, ok + 100, 1 << 30):
        assert product.mat_mix(s.s, bad, ok, 0.5) == RT_EHANDLE
        assert product.mat_mix(s.s, ok, bad, 0.5) == RT_EHANDLE
        assert product.mat_mix_image(s.s, bad, ok, image) == RT_EHANDLE
        assert product.mat_mix_image(s.s, ok, bad, image) == RT_EHANDLE
    for bad in (-2, ok + 100, 1 << 30):  # (-1 is "no wrapped material")
        assert product.mat_diffuse_light(s.s, solid, bad) == RT_EHANDLE
    assert product.mat_diffuse_light(s.s, -1, ok) == RT_EHANDLE
    # Mix::from_image takes an ImageTexture (material.rs:235-247)
    for bad in (solid, noise, -1, image + 100):
        assert product.mat_mix_image(s.s, ok, ok, bad) == RT_EHANDLE
    assert product.mat_mix(s.s, ok, ok, 0.5) >= 0
    assert product.mat_mix_image(s.s, ok, ok, image) >= 0
    assert product.mat_diffuse_light(s.s, solid, ok) >= 0


@pytest.mark.parametrize("name", mw.FURNACE)
def test_oracle_furnace(oracle, rt, name):
    """f / pdf of SpherePDF and CosinePDF at albedo 1 is x / x, Transparent and
    a white Dielectric carry 1: every sample is exactly 1."""
    s = rt.Scene(oracle)
    world, lights, cam = mw.build(rt, s, "furnace_" + name)
    lin, _, st = cam.render(world, lights, seed=1, want_srgb=False)
    assert st.panics == 0
    assert np.all(lin == 1.0)


@pytest.mark.parametrize("name", sorted(mw.EMISSION))
def test_oracle_emission(oracle, rt, name):
    """DiffuseLight's own colour plus its wrapped material's; a Mix of two equal
    lights (0.75 c + 0.25 c, exact in binary)."""
    s = rt.Scene(oracle)
    world, lights, cam = mw.build(rt, s, "emission_" + name)
    lin, _, st = cam.render(world, lights, seed=1, want_srgb=False)
    assert st.panics == 0
    np.testing.assert_array_equal(lin, np.broadcast_to(np.float32(mw.EMISSION[name]), lin.shape))


def _oracle_frame(oracle, rt, name, alter=None):
    s = rt.Scene(oracle)
    world, lights, cam = mw.build(rt, s, name, alter)
    return cam.render(world, lights, seed=1, want_srgb=False)[0]


@pytest.mark.parametrize("name,alter", [(n, "one_table") for n in mw.CASES if n.startswith("noise_")] +
                         [(n, "flat_image") for n in mw.CASES if n.startswith(("uvwrap_", "general_"))])
def test_worlds_tell_a_wrong_lookup_apart(oracle, rt, name, alter):
    """The parity tests can only notice what changes the frame.  A kernel that
    read the first Perlin table for every NoiseTexture, or sampled a wrapped
    image texture at (u, v) = (0, 0) for want of MF_NEEDS_UV, would render
    the altered world (family_materials): on the oracle that frame misses the
    share of pixels within 1e-5 that test_parity_gpu.check asks for."""
    o, a = _oracle_frame(oracle, rt, name), _oracle_frame(oracle, rt, name, alter)
    exact = np.mean(np.all(np.abs(a - o) <= 1e-5 * np.maximum(1.0, np.abs(o)), axis=-1))
    print(name, alter, "pixels within 1e-5 of the true world's:", exact)
    assert exact < 0.999


@pytest.mark.parametrize("name", mw.ALL)
def test_oracle_renders_without_panic(oracle, rt, name):
    s = rt.Scene(oracle)
    world, lights, cam = mw.build(rt, s, name)
    lin, _, st = cam.render(world, lights, seed=1, want_srgb=False)
    assert st.panics == 0
    assert np.isfinite(lin).all()
    if name.startswith("ends_"):
        # Mix(lamp, L, 1.5) emits (1 - 1.5) * lamp: negative radiance, unclamped (material.rs:262-266)
        assert lin.min() < 0.0
