"""rt_world_hit without a device: the argument checks of the product's two
entry points, the two structures' sizes, the oracle's hit-query driver
(tests/cpp/hit_query_oracle.cpp) against closed forms, and -- on the driver
alone -- that every ray set tests/test_world_hit_gpu.py sends is what it is
meant to be: at least 10 % hits and 10 % misses, a hit of every primitive kind
the world holds, back-face hits from points inside its closed shapes, media
both hit and passed through, and the kernel tier the world is meant to select.
"""
import ctypes as C
import math
import tempfile

import numpy as np
import pytest

import hit_query as hq

INF = float("inf")
EINVAL, EHANDLE, EMOVED, EDEVICE = -1, -2, -3, -7


def test_structures_have_the_abi_sizes(capi, rt):
    assert C.sizeof(capi.RtRay) == 64
    assert C.sizeof(capi.RtHitRecord) == 80
    assert rt.HIT_DTYPE.itemsize == 80
    assert [rt.HIT_DTYPE.fields[k][1] for k in ("t", "p", "normal", "u", "v", "mat", "flags")] == [0, 8, 32, 56, 64, 72, 76]


def _one_sphere(rt, api):
    s = rt.Scene(api)
    m = s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, -5.0), 1.0, m))
    return s, w, m


def _call(api, s, world_h, rays, n=None, flags=0, out=True):
    capi = hq.pkg_module("capi")
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    n = len(a) if n is None else n
    rec = (capi.RtHitRecord * max(len(a), 1))()
    return api.world_hit(s.s if s is not None else None, world_h, 0, flags,
                         a.ctypes.data_as(C.POINTER(capi.RtRay)) if rays is not None else None, n,
                         rec if out else None)


GOOD = [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, INF]


def test_argument_checks(product, rt, capi):
    s, w, _ = _one_sphere(rt, product)
    # n == 0: RT_OK, no device touched, no arrays needed -- in both variants
    assert product.world_hit(s.s, w.h, 0, 0, None, 0, None) == 0
    assert product.world_hit_device(s.s, w.h, 0, 0, None, 0, None, None) == 0
    assert product.world_hit(s.s, w.h, 0, 1, None, 0, None) == 0  # RT_FLAG_REFERENCE_BVH
    # null scene or arrays
    assert _call(product, None, w.h, [GOOD]) == EINVAL
    assert _call(product, s, w.h, [GOOD], out=False) == EINVAL
    assert product.world_hit(s.s, w.h, 0, 0, None, 1, (capi.RtHitRecord * 1)()) == EINVAL
    assert product.world_hit_device(s.s, w.h, 0, 0, None, 1, None, None) == EINVAL
    assert product.world_hit_device(s.s, w.h, 0, 0, C.c_void_p(64), 1, None, None) == EINVAL
    # n >= 2^32 (refused before an array is read)
    assert _call(product, s, w.h, [GOOD], n=1 << 32) == EINVAL
    assert product.world_hit_device(s.s, w.h, 0, 0, C.c_void_p(64), 1 << 32, C.c_void_p(64), None) == EINVAL
    assert b"2^32" in product.last_error()
    # flags other than RT_FLAG_REFERENCE_BVH
    for bad in (2, 3, 0x80000000):
        assert _call(product, s, w.h, [GOOD], flags=bad) == EINVAL
        assert product.world_hit_device(s.s, w.h, 0, bad, C.c_void_p(64), 1, C.c_void_p(64), None) == EINVAL
    # handles: unknown, and moved into another object
    for h in (-1, 9999):
        assert _call(product, s, h, [GOOD]) == EHANDLE
        assert product.world_hit_device(s.s, h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EHANDLE
    outer = s.Hittables()
    outer.add(w)
    assert _call(product, s, w.h, [GOOD]) == EMOVED
    assert product.world_hit_device(s.s, w.h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EMOVED


@pytest.mark.parametrize("field, value", [(0, math.nan), (1, INF), (2, -INF), (3, math.nan), (4, INF), (5, -INF),
                                          (6, math.nan), (6, INF), (7, math.nan), (7, -1.0), (7, -INF)])
def test_host_variant_refuses_a_bad_ray(product, rt, field, value):
    s, w, _ = _one_sphere(rt, product)
    rays = [GOOD, GOOD, GOOD]
    rays[1] = list(GOOD)
    rays[1][field] = value
    assert _call(product, s, w.h, rays) == EINVAL
    assert b"ray 1" in product.last_error()


def test_host_variant_refuses_a_zero_direction(product, rt):
    s, w, _ = _one_sphere(rt, product)
    assert _call(product, s, w.h, [GOOD, [1.0, 2.0, 3.0, 0.0, -0.0, 0.0, 0.0, INF]]) == EINVAL


def test_no_device_is_an_error_not_a_fallback(product, rt):
    """n > 0 needs a gfx950 device: RT_EDEVICE without one, never a CPU answer."""
    import torch
    s, w, _ = _one_sphere(rt, product)
    rc = _call(product, s, w.h, [GOOD])
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc == EDEVICE, product.last_error()
        assert product.world_hit_device(s.s, w.h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EDEVICE


# ---------------------------------------------------------------- the driver against closed forms
def test_driver_sphere_closed_forms(rt):
    drv = hq.driver(True)
    s, w, m = _one_sphere(rt, drv)
    rays = np.array([
        [0, 0, 0, 0, 0, -1, 0, INF],                      # t = 4 on the near side
        [0, 0, 0, 0, 0, -2, 0, INF],                      # the direction is not normalised: t = 2
        [0, 0, -5, 0, 0, -1, 0, INF],                     # from the centre: the far root, back face
        [0, 0, 0, 0, 0, -1, 0, 3.9],                      # t_max below the hit
        [0, 0, 0, 0, 0, -1, 0, 4.0],                      # at it: the interval is closed
        [0, 0, 0, 0, 0, -1, 0, np.nextafter(4.0, 0.0)],   # one ulp under it
        [0, 0, 0, 0, 1, 0, 0, INF],                       # away from it
        [0, 0, -4 + 1e-9, 0, 0, 1, 0, INF],               # leaving the surface from just inside: t = 1e-9 < t_min
    ], dtype=np.float64)
    r = hq.oracle_hit(drv, s, w, rays)
    assert list(r["flags"]) == [3, 3, 1, 0, 3, 0, 0, 0]
    assert list(r["t"][:3]) == [4.0, 2.0, 1.0] and r["t"][4] == 4.0
    np.testing.assert_array_equal(r["p"][:3], [[0, 0, -4], [0, 0, -4], [0, 0, -6]])
    # the unit normal faces the ray: outward on the near side, flipped inside
    np.testing.assert_array_equal(r["normal"][:3], [[0, 0, 1], [0, 0, 1], [0, 0, 1]])
    # sphere.rs:53-61: u = (atan2(-z, x) + pi) / 2 pi, v = acos(-y) / pi of the outward normal
    assert r["u"][0] == 0.25 and r["v"][0] == 0.5 and r["u"][2] == 0.75 and r["v"][2] == 0.5
    assert list(r["mat"]) == [m.h, m.h, m.h, -1, m.h, -1, -1, -1]
    miss = r[3]
    assert miss["t"] == 0 and not miss["p"].any() and not miss["normal"].any() and miss["u"] == 0 and miss["v"] == 0


def test_driver_quad_closed_forms(rt):
    drv = hq.driver(True)
    s = rt.Scene(drv)
    m0 = s.Lambertian(s.SolidColor((0.1, 0.2, 0.3)))
    m = s.Metal((0.7, 0.6, 0.5), 0.0)
    w = s.Hittables()
    w.add(s.Quad((-1.0, -1.0, -3.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), m))
    rays = np.array([
        [0.5, 0.25, 0, 0, 0, -1, 0, INF],    # front: alpha = 0.75, beta = 0.625
        [0.5, 0.25, -6, 0, 0, 1.5, 0, INF],  # from behind: t = 2, the normal turned
        [0.5, 0.25, 0, 0, 0, -1, 0, 1.5],    # t_max below
        [0.5, 0.25, 0, 0, 0, -1, 0, 3.0],    # at
        [0.5, 0.25, 0, 0, 0, -1, 0, np.nextafter(3.0, 0.0)],
        [1.5, 0.25, 0, 0, 0, -1, 0, INF],    # past the edge
        [0.5, 0.25, 0, 1, 0, 0, 0, INF],     # parallel to the plane
    ], dtype=np.float64)
    r = hq.oracle_hit(drv, s, w, rays)
    assert list(r["flags"]) == [3, 1, 0, 3, 0, 0, 0]
    assert list(r["t"][:2]) == [3.0, 2.0] and r["t"][3] == 3.0
    np.testing.assert_array_equal(r["p"][:2], [[0.5, 0.25, -3], [0.5, 0.25, -3]])
    np.testing.assert_array_equal(r["normal"][:2], [[0, 0, 1], [0, 0, -1]])
    assert list(r["u"][:2]) == [0.75, 0.75] and list(r["v"][:2]) == [0.625, 0.625]
    assert m.h != m0.h and list(r["mat"]) == [m.h, m.h, -1, m.h, -1, -1, -1]


def test_driver_medium_draw_is_keyed_by_seed_and_index(rt):
    """One ray many times through a thin medium: the draw (pixel = the ray's
    index) lets some through, and another seed others."""
    drv = hq.driver(True)
    s = rt.Scene(drv)
    w = s.Hittables()
    w.add(s.ConstantMedium(s.Sphere((0.0, 0.0, -5.0), 1.0, s.EmptyMaterial()), 0.5, s.SolidColor((1, 1, 1))))
    rays = np.tile(np.array([0, 0, 0, 0, 0, -1, 0, INF], dtype=np.float64), (256, 1))
    a, b = hq.oracle_hit(drv, s, w, rays, seed=1), hq.oracle_hit(drv, s, w, rays, seed=2)
    hit = (a["flags"] & hq.FOUND) != 0
    assert 0.3 < hit.mean() < 0.9  # 1 - exp(-0.5 * 2) = 0.63
    assert np.all((a["flags"][hit] & hq.MEDIUM) != 0) and np.all(a["mat"] == -1)
    # volume.rs:67-72 hands HitRecord::new the normal (1, 0, 0), which turns it against the
    # ray like any other (hit.rs:33-36): d.x = 0 is no front face, so the record holds its negative
    assert not np.any(a["flags"] & hq.FRONT)
    np.testing.assert_array_equal(a["normal"][hit], np.tile([-1.0, -0.0, -0.0], (hit.sum(), 1)))
    toward = rays.copy()
    toward[:, 3] = -0.05
    c = hq.oracle_hit(drv, s, w, toward, seed=1)
    chit = (c["flags"] & hq.FOUND) != 0
    assert chit.any() and np.all((c["flags"][chit] & hq.FRONT) != 0)
    np.testing.assert_array_equal(c["normal"][chit], np.tile([1.0, 0.0, 0.0], (chit.sum(), 1)))
    assert not a["u"].any() and not a["v"].any()
    assert np.all((a["t"][hit] >= 4.0) & (a["t"][hit] <= 6.0)) and len(np.unique(a["t"][hit])) == hit.sum()
    assert np.any(a["flags"] != b["flags"])
    np.testing.assert_array_equal(hq.oracle_hit(drv, s, w, rays, seed=1), a)


# ---------------------------------------------------------------- the GPU test's ray sets
@pytest.mark.parametrize("name", sorted(hq.WORLDS))
def test_ray_sets_are_what_they_are_meant_to_be(product, capi, name):
    build, flags, tier, kinds, media = hq.WORLDS[name]
    rays, where, rec = hq.reference(name)
    found = (rec["flags"] & hq.FOUND) != 0
    medium = (rec["flags"] & hq.MEDIUM) != 0
    print(f"{name}: {len(rays)} rays, {found.mean():.2f} hit, {int(medium.sum())} medium hits")
    assert np.all(np.isfinite(rays[:, :7])) and np.all(rays[:, 7] >= 0) and np.all(np.any(rays[:, 3:6] != 0, axis=1))
    assert found.mean() >= 0.10 and (~found).mean() >= 0.10
    # the product's view of the same world: the tier it selects (host only)
    s, w, cam, extras, _, _ = hq.world_case(product, name, tempfile.mkdtemp(prefix="hit_world_"))
    assert hq.kinds_hit(rec, extras) >= set(kinds), hq.kinds_hit(rec, extras)
    # rays from inside a closed shape: every world has them, and they see a surface's back
    # (a point inside a medium's boundary sees the medium and the room, which is no back face)
    inside = [p for p in where if p.startswith("inside")]
    assert len(inside) == len(extras["inside"]) >= 1
    backs = {}
    for p in inside:
        f = rec[where[p]]["flags"]
        backs[p] = int((((f & hq.FOUND) != 0) & ((f & (hq.FRONT | hq.MEDIUM)) == 0)).sum())
        print(f"  {p} {extras['inside'][int(p[6:])]}: {backs[p]} of {len(f)} back-face hits")
    assert any(backs.values()), backs
    if not media:
        assert all(backs.values()), backs
    info = capi.RtWorldInfo()
    product.check(product.world_info_get(s.s, w.h, -1, -1, flags, C.byref(info)))
    assert info.kernel_tier == tier, info.kernel_tier
    if name == "big_spheres":  # its tree leaves the basic tier's LDS copy (RT_NODE_LDS_BYTES / 112 = 658 nodes)
        assert info.bvh_nodes > 658 and info.primitives > 2500
    if name == "wide":
        assert 365 < info.bvh_nodes <= 658
    if media:
        # hit in the medium, and through it onto what lies behind or out of the world
        assert medium.sum() >= 50 and (found & ~medium).sum() >= 50
        g = where["grid"]
        assert medium[g].any() and (found[g] & ~medium[g]).any()
    else:
        assert not medium.any()
    # a solid surface's first hit survives t_max = t and not one ulp less (a medium's
    # hit moves with t_max and the ray's index: volume.rs:58-65)
    g = where["grid"]
    solid = (found[g] & ~medium[g])[found[g]]
    at, under = rec[where["tmax_at"]], rec[where["tmax_under"]]
    if not media:
        assert np.all((at["flags"] & hq.FOUND) != 0) and not np.any(under["flags"] & hq.FOUND)
        np.testing.assert_array_equal(at["t"], rec[g]["t"][found[g]])
        assert not np.any(rec[where["tmax_half"]]["flags"] & hq.FOUND)
    else:
        assert solid.any()
    if extras.get("moving"):
        # the moving sphere is somewhere else at another time
        t0, t1 = rec[g][::3], rec[where["time_one"]]
        assert np.any(t0["t"] != t1["t"])
