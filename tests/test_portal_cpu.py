"""The Portal material without a GPU: the rt_mat_portal ABI and its flattening
(F_PORTAL, tier 4, or 5 beside a Disney material; wrappers; the Transparent
twin untouched), and the test-side restatement (tests/cpp/portal_oracle.cpp)
checked against the oracle itself: a Portal that moves and turns nothing is a
Transparent.  Fidelity to portal.rs otherwise rests on review of the cited
lines: the reference cannot be run here.
"""
import ctypes as C
import math

import numpy as np
import pytest

import portal_query as pq

_DP = C.POINTER(C.c_double)


def _d(*v):
    return (C.c_double * len(v))(*v)


# ---------------------------------------------------------------- ABI
@pytest.mark.parametrize("which", ["product", "restatement"])
def test_error_codes(product, rt, which):
    """RT_EINVAL for a null scene, a null attenuation and any non-finite value;
    null offset and null quaternion give a handle; nothing else is checked."""
    api = product if which == "product" else pq.driver()
    s = rt.Scene(api)
    white, off, q = _d(1.0, 1.0, 1.0), _d(2.0, 0.0, 0.0), _d(1.0, 0.0, 0.0, 0.0)
    assert api.mat_portal(s.s, white, off, q) >= 0
    assert api.mat_portal(s.s, white, None, q) >= 0
    assert api.mat_portal(s.s, white, off, None) >= 0
    assert api.mat_portal(s.s, white, None, None) >= 0
    assert api.mat_portal(None, white, off, q) == -1
    assert api.mat_portal(s.s, None, off, q) == -1
    for bad in (math.nan, math.inf, -math.inf):
        for k in range(3):
            a = [1.0, 1.0, 1.0]
            a[k] = bad
            assert api.mat_portal(s.s, _d(*a), off, q) == -1, (bad, k)
            o = [2.0, 0.0, 0.0]
            o[k] = bad
            assert api.mat_portal(s.s, white, _d(*o), q) == -1, (bad, k)
        for k in range(4):
            r = [1.0, 0.0, 0.0, 0.0]
            r[k] = bad
            assert api.mat_portal(s.s, white, off, _d(*r)) == -1, (bad, k)
    # a zero or non-unit quaternion, a negative attenuation: accepted, as the reference checks nothing
    assert api.mat_portal(s.s, white, off, _d(0.0, 0.0, 0.0, 0.0)) >= 0
    assert api.mat_portal(s.s, _d(-1.0, 2.0, 0.0), off, _d(0.5, 0.5, 0.5, 0.7)) >= 0
    # and the mirror's handles are materials like any other
    m = s.Portal((1.0, 1.0, 1.0))
    assert s.Sphere((0.0, 0.0, 0.0), 1.0, m).h >= 0


# ---------------------------------------------------------------- flattening
def _info(api, capi, s, world, lights=None, bg=None):
    info = capi.RtWorldInfo()
    api.check(api.world_info_get(s.s, world.h, -1 if lights is None else lights.h, -1 if bg is None else bg.h, 0,
                                 C.byref(info)))
    return info


def _one_sphere(s, mat):
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, 0.0), 1.0, mat))
    return w


def test_world_info_tier_and_feature(product, capi, rt):
    """A Portal world reports F_PORTAL and tier 4, with a Disney material as
    well tier 5; the twin with Transparent in the Portal's place reports what
    it reports without this material."""
    f_portal, f_disney = pq.feature_bit("F_PORTAL"), pq.feature_bit("F_DISNEY")
    assert f_portal == 2048
    s = rt.Scene(product)
    tex = s.SolidColor((0.8, 0.8, 0.8))
    p = _info(product, capi, s, _one_sphere(s, s.Portal((1.0, 1.0, 1.0), (2.0, 0.0, 0.0))))
    assert p.kernel_tier == 4 and p.features & f_portal and not p.features & f_disney
    t = _info(product, capi, s, _one_sphere(s, s.Transparent()))
    assert t.kernel_tier == 3 and not t.features & f_portal  # (Transparent: a full tier; no BVH node: the flat one)
    assert (p.primitives, p.stack_need) == (t.primitives, t.stack_need)
    # both: the Disney tier
    w = _one_sphere(s, s.Portal((1.0, 1.0, 1.0)))
    w.add(s.Sphere((3.0, 0.0, 0.0), 1.0, s.Disney(tex)))
    both = _info(product, capi, s, w)
    assert both.kernel_tier == 5 and both.features & f_portal and both.features & f_disney
    # an unused Portal does not move the tier
    lam = _info(product, capi, s, _one_sphere(s, s.Lambertian(tex)))
    assert lam.kernel_tier == 0 and not lam.features & f_portal


@pytest.mark.parametrize("name", list(pq.WORLDS))
def test_render_worlds_tiers_and_twins(product, capi, rt, name):
    """The GPU tests' worlds take the tier stated; their Transparent twins
    report no F_PORTAL and the tier they took before (below 4 unless another
    material asks for more)."""
    f_portal = pq.feature_bit("F_PORTAL")
    s = rt.Scene(product)
    world, lights, cam = pq.WORLDS[name](s)
    info = _info(product, capi, s, world, lights, cam.background)
    assert info.kernel_tier == pq.TIERS[name] and info.features & f_portal
    s2 = rt.Scene(product)
    world2, lights2, cam2 = pq.WORLDS[name](s2, portal=False)
    twin = _info(product, capi, s2, world2, lights2, cam2.background)
    assert not twin.features & f_portal
    # (Transparent is a full-tier material, F_MATFULL; a Portal asks for its own bit only)
    f_matfull = pq.feature_bit("F_MATFULL")
    assert twin.features | f_matfull == (info.features & ~f_portal) | f_matfull
    assert twin.kernel_tier == {"scene": 3, "rotated": 2, "wrapped": 5}[name]
    assert (twin.primitives, twin.bvh_leaves) == (info.primitives, info.bvh_leaves)


def test_tier_for_keeps_every_other_combination(product):
    """tier_for with F_PORTAL: 5 beside F_DISNEY, else 4; without it what it returned before."""
    names = ("F_XFORM", "F_MEDIUM", "F_PLANAR", "F_MSPHERE", "F_LIGHTS", "F_TEXFULL", "F_MATFULL", "F_REMAP", "F_NORMALMAP",
             "F_GENERAL", "F_DISNEY")
    bit = {n: pq.feature_bit(n) for n in names}
    f_portal = pq.feature_bit("F_PORTAL")
    assert f_portal not in bit.values()
    full = sum(bit[n] for n in ("F_XFORM", "F_MEDIUM", "F_MSPHERE", "F_LIGHTS", "F_TEXFULL", "F_MATFULL", "F_NORMALMAP"))
    fn = product.lib.rtk_tier_for
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32]
    for f in range(2048):
        want = (5 if f & bit["F_DISNEY"] else 4 if f & bit["F_GENERAL"] else 2 if f & full
                else 1 if f & (bit["F_PLANAR"] | bit["F_REMAP"]) else 0)
        assert fn(f) == want, f
        assert fn(f | f_portal) == (5 if f & bit["F_DISNEY"] else 4), f


def test_portal_under_wrappers(product, capi, rt):
    """A Portal reachable only through Mix, Mix::from_image or DiffuseLight(tex,
    inner) sets the bit; the Transparent twin of each does not; five wrapper
    levels are still refused."""
    f_portal = pq.feature_bit("F_PORTAL")
    s = rt.Scene(product)
    tex = s.SolidColor((0.8, 0.8, 0.8))
    lam = s.Lambertian(tex)
    img = s.ImageTexture(np.full((2, 2, 4), 0.5, dtype=np.float32))
    for is_portal in (True, False):
        inner = s.Portal((0.9, 0.9, 0.9), (1.0, 0.0, 0.0)) if is_portal else s.Transparent()
        for m in (s.Mix(inner, lam, 0.5), s.Mix(lam, inner, 0.5), s.Mix_from_image(lam, inner, img), s.DiffuseLight(tex, inner),
                  s.Mix(lam, s.DiffuseLight(tex, s.Mix(lam, inner, 0.25)), 0.5)):
            info = _info(product, capi, s, _one_sphere(s, m))
            assert bool(info.features & f_portal) == is_portal, (is_portal, m.h)
            if is_portal:
                assert info.kernel_tier == 4
    m = s.Portal((1.0, 1.0, 1.0))
    for _ in range(4):
        m = s.DiffuseLight(tex, m)
    deep = _info(product, capi, s, _one_sphere(s, m))
    assert deep.kernel_tier == 4 and deep.features & f_portal
    m = s.DiffuseLight(tex, m)
    info = capi.RtWorldInfo()
    assert product.world_info_get(s.s, _one_sphere(s, m).h, -1, -1, 0, C.byref(info)) == -6


def test_portal_record_is_not_a_material_link(product, capi, rt):
    """DMaterial::inner of a Portal indexes its DPortal record, not a material:
    the first Portal's index 0 must not mark material 0 used (here a
    Lambertian with an image texture, which would pull F_TEXFULL in)."""
    f_texfull = pq.feature_bit("F_TEXFULL")
    s = rt.Scene(product)
    img = s.ImageTexture(np.full((2, 2, 4), 0.5, dtype=np.float32))
    lit = s.Lambertian(img)  # material 0: what a Portal's record index 0 would name as a material
    assert lit.h == 0
    p = _info(product, capi, s, _one_sphere(s, s.Portal((1.0, 1.0, 1.0))))
    assert p.kernel_tier == 4 and not p.features & f_texfull


# ---------------------------------------------------------------- the restatement
def test_null_portal_is_transparent_on_the_restatement():
    """Portal(WHITE, 0, identity) renders the `scene` world bit-equal to
    Transparent on the extended oracle: (q * qv) * conj(q) with q = 1 is exact
    for non-zero components, rec.p + 0 is rec.p and WHITE * x is x.  (Seed 1
    meets no -0.0 direction component on the quad: a +0.0 would come back
    from it, and the frames would still agree unless a later division by it
    chose a side.)"""
    a = pq.reference("scene", null_portal=True)
    b = pq.reference("scene", portal=False)
    assert a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes()
    assert a[2].tobytes() == b[2].tobytes()
    assert a[3] == b[3] == 0
    # and the portal proper shows something else: its quad looks down on the sphere
    c = pq.reference("scene")
    assert c[0].tobytes() != b[0].tobytes()


@pytest.mark.parametrize("name", list(pq.WORLDS))
def test_render_worlds_on_the_restatement(name):
    """The GPU tests' worlds render finite frames that differ from their Transparent twins."""
    lin, srgb, part, panics = pq.reference(name)
    assert np.isfinite(lin).all() and lin.shape == (18, 32, 3) and lin.max() > 0.05
    assert part.shape == (18, 32, 4, 3)
    twin = pq.reference(name, portal=False)
    assert lin.tobytes() != twin[0].tobytes()
    print(f"{name}: panics on the restatement {panics}, mean radiance {lin.mean():.4f} (twin {twin[0].mean():.4f})")
