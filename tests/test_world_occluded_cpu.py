"""rt_world_occluded without a device: the argument checks of the product's two
entry points, as tests/test_world_hit_cpu.py makes them for rt_world_hit, and
-- on the oracle's hit-query driver alone -- that the ray sets
tests/test_world_occluded_gpu.py sends are worth testing an any-hit query on:
a fifth to a half of every set occluded, the t_max cases on either side of
the first hit, and in the media worlds rays that a medium blocks.
"""
import ctypes as C
import math

import numpy as np
import pytest

import hit_query as hq

INF = float("inf")
EINVAL, EHANDLE, EMOVED, EDEVICE = -1, -2, -3, -7
GOOD = [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, INF]


def _one_sphere(rt, api):
    s = rt.Scene(api)
    m = s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, -5.0), 1.0, m))
    return s, w


def _call(api, s, world_h, rays, n=None, flags=0, out=True):
    capi = hq.pkg_module("capi")
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    n = len(a) if n is None else n
    buf = (C.c_uint8 * max(len(a), 1))()
    return api.world_occluded(s.s if s is not None else None, world_h, 0, flags,
                              a.ctypes.data_as(C.POINTER(capi.RtRay)) if rays is not None else None, n,
                              buf if out else None)


def test_argument_checks(product, rt, capi):
    s, w = _one_sphere(rt, product)
    dev = product.world_occluded_device
    # n == 0: RT_OK, no device touched, no arrays needed -- in both variants, with either flag
    for flags in (0, 1):  # 1: RT_FLAG_REFERENCE_BVH
        assert product.world_occluded(s.s, w.h, 0, flags, None, 0, None) == 0
        assert dev(s.s, w.h, 0, flags, None, 0, None, None) == 0
    # null scene or arrays
    assert _call(product, None, w.h, [GOOD]) == EINVAL
    assert dev(None, w.h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EINVAL
    assert _call(product, s, w.h, [GOOD], out=False) == EINVAL
    assert product.world_occluded(s.s, w.h, 0, 0, None, 1, (C.c_uint8 * 1)()) == EINVAL
    assert dev(s.s, w.h, 0, 0, None, 1, None, None) == EINVAL
    assert dev(s.s, w.h, 0, 0, C.c_void_p(64), 1, None, None) == EINVAL
    assert dev(s.s, w.h, 0, 0, None, 1, C.c_void_p(64), None) == EINVAL
    # n >= 2^32 (refused before an array is read)
    assert _call(product, s, w.h, [GOOD], n=1 << 32) == EINVAL
    assert b"2^32" in product.last_error()
    assert dev(s.s, w.h, 0, 0, C.c_void_p(64), 1 << 32, C.c_void_p(64), None) == EINVAL
    assert b"2^32" in product.last_error()
    # flags other than RT_FLAG_REFERENCE_BVH
    for bad in (2, 3, 0x80000000):
        assert _call(product, s, w.h, [GOOD], flags=bad) == EINVAL
        assert dev(s.s, w.h, 0, bad, C.c_void_p(64), 1, C.c_void_p(64), None) == EINVAL
    # handles: unknown, and moved into another object
    for h in (-1, 9999):
        assert _call(product, s, h, [GOOD]) == EHANDLE
        assert dev(s.s, h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EHANDLE
    outer = s.Hittables()
    outer.add(w)
    assert _call(product, s, w.h, [GOOD]) == EMOVED
    assert dev(s.s, w.h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EMOVED


@pytest.mark.parametrize("field, value", [(0, math.nan), (1, INF), (2, -INF), (3, math.nan), (4, INF), (5, -INF),
                                          (6, math.nan), (6, INF), (7, math.nan), (7, -1.0), (7, -INF)])
def test_host_variant_refuses_a_bad_ray(product, rt, field, value):
    s, w = _one_sphere(rt, product)
    rays = [GOOD, GOOD, GOOD]
    rays[1] = list(GOOD)
    rays[1][field] = value
    assert _call(product, s, w.h, rays) == EINVAL
    assert b"ray 1" in product.last_error()


def test_host_variant_refuses_a_zero_direction(product, rt):
    s, w = _one_sphere(rt, product)
    assert _call(product, s, w.h, [GOOD, [1.0, 2.0, 3.0, 0.0, -0.0, 0.0, 0.0, INF]]) == EINVAL
    assert b"ray 1" in product.last_error()


def test_no_device_is_an_error_not_a_fallback(product, rt):
    """n > 0 needs a gfx950 device: RT_EDEVICE without one, never a CPU answer."""
    import torch
    s, w = _one_sphere(rt, product)
    rc = _call(product, s, w.h, [GOOD])
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc == EDEVICE, product.last_error()
        assert product.world_occluded_device(s.s, w.h, 0, 0, C.c_void_p(64), 1, C.c_void_p(64), None) == EDEVICE


def test_scene_occluded_refuses_a_wrong_shape(product, rt):
    """Scene.occluded takes Scene.hit's (n, 8) array and raises its ValueError."""
    s, w = _one_sphere(rt, product)
    for bad in (np.zeros(8), np.zeros((3, 7)), np.zeros((2, 8, 1)), np.zeros((0, 9))):
        with pytest.raises(ValueError, match=r"\(n, 8\)"):
            s.occluded(w, bad)
        with pytest.raises(ValueError, match=r"\(n, 8\)"):
            s.hit(w, bad)
    out = s.occluded(w, np.zeros((0, 8)))  # no ray: no device needed
    assert out.shape == (0,) and out.dtype == np.uint8


# ---------------------------------------------------------------- the GPU test's ray sets, on the driver alone
@pytest.mark.parametrize("name", sorted(hq.WORLDS))
def test_ray_sets_are_worth_an_any_hit_query(name):
    _, _, _, _, media = hq.WORLDS[name]
    rays, where, rec = hq.reference(name, 0)
    found = (rec["flags"] & hq.FOUND) != 0
    medium = (rec["flags"] & hq.MEDIUM) != 0
    print(f"{name}: {len(rays)} rays, occluded fraction {found.mean():.3f}, medium blockers {medium.mean():.3f}")
    assert 0.2 <= found.mean() <= 0.55
    if not media:
        assert not found[where["tmax_half"]].any() and not found[where["tmax_under"]].any()
        assert found[where["tmax_at"]].all()
        assert not medium.any()
    else:
        # rays whose blocker is a medium (an any-hit query that ignored media would let them
        # through), rays a surface blocks, and rays nothing blocks
        assert (found & medium).sum() >= 50 and (found & ~medium).sum() >= 50 and (~found).sum() >= 50
        assert np.all(found[medium])
