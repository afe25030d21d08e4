"""rt_wavefront_load_flags on the CPU: the flag contract against the old entry
point, the reference's own mc.obj loading from its own mc.mtl as Disney BSDFs
(obj.rs:279-292), the refusal of non-finite parameters on the product and on
the oracle extension (tests/cpp/obj_disney_oracle.cpp), the eight-key MTL
mapping pinned differentially on the oracle extension, and
scenes.obj_scene / disney_scene / background_scene building on both.

Every test here needs the new entry point or the new scene builders."""
import ctypes
import os
import tempfile

import pytest

import hit_query as hq
import obj_disney_query as oq

EINVAL, EUNSUPPORTED = -1, -6


@pytest.fixture(scope="module")
def drv():
    return oq.driver()


def _load(api, s, path, flags):
    return api.wavefront_load_flags(s.s, os.fsencode(path), flags)


def _info(api, capi, s, h):
    info = capi.RtWorldInfo()
    api.check(api.world_info_get(s.s, h, -1, -1, 0, ctypes.byref(info)))
    return tuple(getattr(info, f) for f, _ in capi.RtWorldInfo._fields_ if f != "device_bytes")


def test_unknown_flag_bits_are_einval(product, drv, rt):
    path = os.path.join(oq.REF_ASSETS, "镜子.obj")
    for api in (product, drv):
        s = rt.Scene(api)
        for flags in (4, 8 | oq.OBJ_DISNEY, 0x80000000 | oq.OBJ_VANILLA):
            assert _load(api, s, path, flags) == EINVAL, flags
            assert b"flags" in api.last_error()


@pytest.mark.parametrize("name", ["镜子.obj", "水面.obj"])
def test_without_the_disney_flag_it_is_the_old_entry_point(product, drv, rt, capi, name):
    """Flags 0 and RT_OBJ_VANILLA: rt_wavefront_load(vanilla = 0 / 1), its
    rt_world_info on the reference's vanilla assets (vanilla = 0 refuses them:
    their materials are then Disney's)."""
    path = os.path.join(oq.REF_ASSETS, name)
    s_old, s_new = rt.Scene(product), rt.Scene(product)
    old = product.check(product.wavefront_load(s_old.s, os.fsencode(path), 1))
    new = product.check(_load(product, s_new, path, oq.OBJ_VANILLA))
    assert _info(product, capi, s_new, new) == _info(product, capi, s_old, old)
    for api in (product, drv):
        s = rt.Scene(api)
        assert api.wavefront_load(s.s, os.fsencode(path), 0) == EUNSUPPORTED
        old_msg = api.last_error()
        assert _load(api, s, path, 0) == EUNSUPPORTED
        assert api.last_error() == old_msg and b"Disney" in old_msg
        assert _load(api, s, path, oq.OBJ_VANILLA) >= 0


def test_mc_obj_is_still_refused_without_the_flag(product, drv, rt):
    path = os.path.join(oq.REF_ASSETS, "mc.obj")
    for api in (product, drv):
        s = rt.Scene(api)
        for flags in (0, oq.OBJ_VANILLA):
            assert api.wavefront_load(s.s, os.fsencode(path), flags) == EUNSUPPORTED
            old_msg = api.last_error()
            assert _load(api, s, path, flags) == EUNSUPPORTED
            assert api.last_error() == old_msg and b"Disney" in old_msg


def test_mc_loads_from_its_own_mtl(product, drv, rt, capi, tmp_path):
    s = rt.Scene(product)
    world, lights, cam = oq.world_mc(s)
    info = oq.world_info(product, s, world, lights, cam.background)
    assert info.kernel_tier == 5
    want = oq.feature_bits("F_DISNEY", "F_REMAP")
    assert info.features & want == want
    # the same mesh under world_mc_obj's metal MTL
    sm = rt.Scene(product)
    metal, mcam, _ = hq.world_mc_obj(rt, sm, str(tmp_path))
    assert info.primitives == oq.world_info(product, sm, metal).primitives > 500
    # both flag sets, on both sides (no material of mc.mtl is a vanilla one: Pm 0, no Tf)
    for api in (product, drv):
        for flags in (oq.OBJ_DISNEY, oq.OBJ_DISNEY | oq.OBJ_VANILLA):
            assert _load(api, rt.Scene(api), os.path.join(oq.mc_dir(), "mc.obj"), flags) >= 0, api.last_error()
    # the whole file as the reference ships it loads too (the stone objects included)
    assert _load(product, rt.Scene(product), os.path.join(oq.REF_ASSETS, "mc.obj"), oq.OBJ_DISNEY) >= 0


def test_vanilla_arms_come_first(product, rt, capi, tmp_path):
    """RT_OBJ_VANILLA | RT_OBJ_DISNEY: Pm 1 is a Metal and Tf 1 a Dielectric
    (no Disney in the world: a lower tier), anything else a Disney."""
    cases = (({"Pm": "1"}, False), ({"Tf": "1 1 1"}, False), ({"Pm": "0.5"}, True), ({}, True))
    for k, (keys, disney) in enumerate(cases):
        s = rt.Scene(product)
        p = oq.write_tri(str(tmp_path / ("case%d" % k)), keys)
        h = product.check(_load(product, s, p, oq.OBJ_VANILLA | oq.OBJ_DISNEY))
        info = capi.RtWorldInfo()
        product.check(product.world_info_get(s.s, h, -1, -1, 0, ctypes.byref(info)))
        assert bool(info.features & oq.feature_bits("F_DISNEY")) == disney, keys
        assert (info.kernel_tier == 5) == disney, keys


@pytest.mark.parametrize("keys,named", [({"Tf": ""}, b"Tf"), ({"Tf": "x y"}, b"Tf"), ({"Pr": "nan"}, b"Pr"),
                                        ({"Pc": "inf"}, b"Pc")])
def test_non_finite_parameters_are_refused_by_name(product, drv, rt, tmp_path, keys, named):
    """`Tf` with no number is 0 / 0 and `Pr nan` parses as NaN (str::parse::<f64>
    takes "nan" and "inf"): the reference renders NaNs, both sides refuse."""
    p = oq.write_tri(str(tmp_path), keys)
    for api in (product, drv):
        s = rt.Scene(api)
        assert _load(api, s, p, oq.OBJ_DISNEY) == EUNSUPPORTED
        msg = api.last_error()
        assert b"'m'" in msg and b"`" + named + b"`" in msg, msg


def test_a_key_that_does_not_parse_takes_the_default(drv):
    plain = oq.tri_frame(drv, {})[0]
    assert oq.tri_frame(drv, {"Pr": "0.5x", "Pm": "--", "Ps": "1 2"})[0] == plain
    assert oq.tri_frame(drv, {"Pr": "0.25"})[0] != plain


def test_eight_key_mapping_differential_on_the_oracle(drv):
    """An MTL that spells out every default renders the bytes of one that
    omits them; each of the eight keys changed alone changes the frame."""
    moved = oq.differential(drv)
    assert sorted(moved) == sorted(["Pr", "aniso", "Ps", "Pm", "Pc", "Pcr", "Ni", "Tf"])
    assert all(moved.values()), moved


def test_scenes_build_on_product_and_oracle(product, drv, rt, scenes):
    for api in (product, drv):
        for name in ("obj_scene", "disney_scene", "background_scene"):
            world, lights, cam = oq.WORLDS[name](rt.Scene(api))
            assert world.h >= 0 and cam.image_width == oq.WIDTH and cam.background is not None
            assert (lights is None) == (name == "disney_scene")
    s = rt.Scene(product)
    world, lights, cam = oq.world_obj_scene(s)
    info = oq.world_info(product, s, world, lights, cam.background)
    want = oq.feature_bits("F_DISNEY", "F_PORTAL", "F_MEDIUM", "F_XFORM", "F_REMAP", "F_NORMALMAP")
    assert info.kernel_tier == 5 and info.features & want == want, hex(info.features)
    # mc + 2 + 2 mesh triangles, the fog box's 12, the Portal, three boards, the black box's 6 quads, and the
    # two boards of the lights (flattened with the world)
    sm = rt.Scene(product)
    mc = oq.world_info(product, sm, oq.world_mc(sm)[0]).primitives
    assert info.primitives == mc + 4 + 12 + 1 + 3 + 6 + 2
    # (background_scene holds no Disney material and no BVH: the flat tier)
    for name, tier in (("disney_scene", 5), ("background_scene", 3)):
        s = rt.Scene(product)
        world, lights, cam = oq.WORLDS[name](s)
        assert oq.world_info(product, s, world, lights, cam.background).kernel_tier == tier, name


def test_obj_scene_arguments(product, rt, scenes, tmp_path):
    d = oq.small_asset_dir()
    assert len(scenes.OBJ_SCENE_OBJS) == 14 and [v for _, v in scenes.OBJ_SCENE_OBJS].count(True) == 2
    s = rt.Scene(product)
    with pytest.raises(FileNotFoundError):  # the full list: most meshes are not in the small directory
        scenes.obj_scene(s, d)
    with pytest.raises(FileNotFoundError):
        scenes.obj_scene(s, d, objs=oq.SMALL_OBJS, fog="absent.obj")
    # fog=None leaves the medium out; a subset keeps main.rs:312-332's order whatever order it is given in
    world, lights, cam = scenes.obj_scene(s, d, objs=oq.SMALL_OBJS[::-1], fog=None, image_width=oq.WIDTH)
    info = oq.world_info(product, s, world, lights, cam.background)
    assert not info.features & oq.feature_bits("F_MEDIUM")
    assert cam.samples_per_pixel == 3000 and cam.max_depth == 30 and cam.vertical_fov_in_degrees == 23
    s2 = rt.Scene(product)
    w2, l2, c2 = scenes.obj_scene(s2, d, objs=oq.SMALL_OBJS, fog=None, image_width=oq.WIDTH)
    assert oq.world_info(product, s2, w2, l2, c2.background).primitives == info.primitives
