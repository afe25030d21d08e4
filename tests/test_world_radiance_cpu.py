"""rt_world_radiance without a device: the argument checks of the product's
two entry points and the structures' sizes; the oracle's radiance driver
(tests/cpp/radiance_oracle.cpp) pinned to the oracle proper -- on the camera's
own rays it must give the oracle render's f64 frame bit for bit; and, on the
driver alone, that every ray set tests/test_world_radiance_gpu.py sends is
worth the query: the glibc and the correctly rounded builds of the oracle
agree on it, no sample panics, at least a quarter of the rays run two
vertices or more, some miss, some end on a light where the world has one, and
some first hits lie beyond and some within a finite t_max.
"""
import ctypes as C
import math

import numpy as np
import pytest

import material_worlds as mw
import radiance_query as rq

INF = float("inf")
EINVAL, EHANDLE, EMOVED, EDEVICE = -1, -2, -3, -7
GOOD = [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, INF]


def test_structures_have_the_abi_sizes(product, capi, rt):
    assert C.sizeof(capi.RtRadiance) == 32 and rt.RADIANCE_DTYPE.itemsize == 32
    assert [rt.RADIANCE_DTYPE.fields[k][1] for k in ("rgb", "rays", "panics")] == [0, 24, 28]
    assert C.sizeof(capi.RtRadianceOpts) == 40
    o = capi.RtRadianceOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    product.radiance_opts_default(C.byref(o))
    assert (o.struct_size, o.max_depth, o.seed, o.samples, o.flags, o.background_tex, o.first_index, o.stream) == \
        (40, 10, 0, 1, 0, -1, 0, None)
    product.radiance_opts_default(None)  # ignored


def _one_sphere(rt, api):
    s = rt.Scene(api)
    m = s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, -5.0), 1.0, m))
    return s, w


def _opts(product, capi, **over):
    o = capi.RtRadianceOpts()
    product.radiance_opts_default(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _host(product, capi, s, world_h, rays, lights_h=-1, n=None, out=True, opts=True, **over):
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    n = len(a) if n is None else n
    rec = (capi.RtRadiance * max(len(a), 1))()
    o = _opts(product, capi, **over)
    return product.world_radiance(s.s if s is not None else None, world_h, lights_h, C.byref(o) if opts else None,
                                  a.ctypes.data_as(C.POINTER(capi.RtRay)), n, rec if out else None)


def _device(product, capi, s, world_h, lights_h=-1, n=1, rays=64, out=64, opts=True, **over):
    """The device variant with made-up addresses: every check here comes before a device is touched."""
    o = _opts(product, capi, **over)
    return product.world_radiance_device(s.s if s is not None else None, world_h, lights_h,
                                         C.byref(o) if opts else None, C.c_void_p(rays) if rays else None, n,
                                         C.c_void_p(out) if out else None)


def test_argument_checks(product, rt, capi):
    s, w = _one_sphere(rt, product)
    # n == 0: RT_OK, no device touched, no arrays needed -- in both variants
    o = _opts(product, capi)
    assert product.world_radiance(s.s, w.h, -1, C.byref(o), None, 0, None) == 0
    assert product.world_radiance_device(s.s, w.h, -1, C.byref(o), None, 0, None) == 0
    o = _opts(product, capi, flags=1, max_depth=0)  # RT_FLAG_REFERENCE_BVH
    assert product.world_radiance(s.s, w.h, -1, C.byref(o), None, 0, None) == 0
    # null scene, options or arrays
    assert _host(product, capi, None, w.h, [GOOD]) == EINVAL
    assert _host(product, capi, s, w.h, [GOOD], opts=False) == EINVAL
    assert _host(product, capi, s, w.h, [GOOD], out=False) == EINVAL
    assert product.world_radiance(s.s, w.h, -1, C.byref(o), None, 1, (capi.RtRadiance * 1)()) == EINVAL
    assert _device(product, capi, None, w.h) == EINVAL
    assert _device(product, capi, s, w.h, opts=False) == EINVAL
    assert _device(product, capi, s, w.h, rays=0) == EINVAL
    assert _device(product, capi, s, w.h, out=0) == EINVAL
    # struct_size below this version's (options not made by rt_radiance_opts_default)
    for size in (0, 39):
        assert _host(product, capi, s, w.h, [GOOD], struct_size=size) == EINVAL
        assert b"struct_size" in product.last_error()
        assert _device(product, capi, s, w.h, struct_size=size) == EINVAL
    assert _host(product, capi, s, w.h, [], n=0, struct_size=0) == EINVAL  # checked before n == 0 returns
    # samples == 0
    assert _host(product, capi, s, w.h, [GOOD], samples=0) == EINVAL
    assert b"samples" in product.last_error()
    assert _device(product, capi, s, w.h, samples=0) == EINVAL
    # flags other than RT_FLAG_REFERENCE_BVH
    for bad in (2, 3, 0x80000000):
        assert _host(product, capi, s, w.h, [GOOD], flags=bad) == EINVAL
        assert _device(product, capi, s, w.h, flags=bad) == EINVAL
    # first_index + n > 2^32 (refused before an array is read); exactly 2^32 passes this check
    assert _host(product, capi, s, w.h, [GOOD], n=(1 << 32) + 1) == EINVAL
    assert b"2^32" in product.last_error()
    assert _host(product, capi, s, w.h, [GOOD], n=2, first_index=0xFFFFFFFF) == EINVAL
    assert _device(product, capi, s, w.h, n=1 << 32, first_index=1) == EINVAL
    assert _device(product, capi, s, w.h, n=0, first_index=0xFFFFFFFF) == 0
    # handles: unknown world, lights and background, and a world moved into another object
    for h in (-1, 9999):
        assert _host(product, capi, s, h, [GOOD]) == EHANDLE
        assert _device(product, capi, s, h) == EHANDLE
    for h in (-2, 9999):
        assert _host(product, capi, s, w.h, [GOOD], lights_h=h) == EHANDLE
        assert _device(product, capi, s, w.h, lights_h=h) == EHANDLE
        assert _host(product, capi, s, w.h, [GOOD], background_tex=h) == EHANDLE
        assert _device(product, capi, s, w.h, background_tex=h) == EHANDLE
    outer = s.Hittables()
    outer.add(w)
    assert _host(product, capi, s, w.h, [GOOD]) == EMOVED
    assert _device(product, capi, s, w.h) == EMOVED
    assert _host(product, capi, s, outer.h, [GOOD], lights_h=w.h) == EMOVED


@pytest.mark.parametrize("field, value", [(0, math.nan), (1, INF), (2, -INF), (3, math.nan), (4, INF), (5, -INF),
                                          (6, math.nan), (6, INF), (7, math.nan), (7, -1.0), (7, -INF)])
def test_host_variant_refuses_a_bad_ray(product, rt, capi, field, value):
    s, w = _one_sphere(rt, product)
    rays = [GOOD, GOOD, GOOD]
    rays[1] = list(GOOD)
    rays[1][field] = value
    assert _host(product, capi, s, w.h, rays) == EINVAL
    assert b"ray 1" in product.last_error()
    assert _host(product, capi, s, w.h, rays, max_depth=0) == EINVAL  # whatever the depth


def test_host_variant_refuses_a_zero_direction(product, rt, capi):
    s, w = _one_sphere(rt, product)
    assert _host(product, capi, s, w.h, [GOOD, [1.0, 2.0, 3.0, 0.0, -0.0, 0.0, 0.0, INF]]) == EINVAL
    assert b"ray 1" in product.last_error()


def test_wrong_shapes_raise(product, rt):
    s, w = _one_sphere(rt, product)
    for bad in (np.zeros(8), np.zeros((3, 7)), np.zeros((2, 3, 8))):
        with pytest.raises(ValueError, match=r"\(n, 8\)"):
            s.radiance(w, None, bad)
    rgb, rays, panics = s.radiance(w, None, np.zeros((0, 8)))  # n == 0 needs no device
    assert rgb.shape == (0, 3) and rgb.dtype == np.float64
    assert rays.shape == (0,) and rays.dtype == np.uint32 and panics.shape == (0,) and panics.dtype == np.uint32


def test_no_device_is_an_error_not_a_fallback(product, rt, capi):
    """n > 0 needs a gfx950 device: RT_EDEVICE without one, never a CPU answer."""
    import torch
    s, w = _one_sphere(rt, product)
    rc = _host(product, capi, s, w.h, [GOOD])
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc == EDEVICE, product.last_error()
        assert _host(product, capi, s, w.h, [GOOD], max_depth=0) == EDEVICE
        assert _device(product, capi, s, w.h) == EDEVICE
        assert _device(product, capi, s, w.h, max_depth=0) == EDEVICE


# ---------------------------------------------------------------- the driver against the oracle proper
@pytest.mark.parametrize("name", ["plain_bvh_lit", "noise_general"])
def test_driver_gives_the_oracle_render_bit_for_bit(rt, name):
    """A 1-spp frame: ray_color of the camera's own rays, keyed by their pixel,
    is the oracle render's linear frame, to the last bit of every f64."""
    drv = rq.driver(True)
    s = rt.Scene(drv)
    world, lights, cam = mw.build(rt, s, name)
    cam.samples_per_pixel = 1
    seed = 5
    c = cam.to_c()
    opts = rt.Camera._opts(drv, seed, 0, 1, 0, 0)[0]
    W, H = cam.image_width, cam.image_height
    frame = np.zeros((H * W, 3), dtype=np.float64)
    drv.check(drv.render_f64(s.s, world.h, -1 if lights is None else lights.h, C.byref(c), C.byref(opts),
                             frame.ctypes.data_as(C.POINTER(C.c_double)), None, None, None))
    rays = rq.camera_rays(drv, s, cam, seed)
    assert np.all(rays[:, 7] == INF) and np.all((rays[:, 6] >= 0) & (rays[:, 6] < 1))
    rgb, calls, panics = rq.oracle_radiance(drv, s, world, lights, rays, max_depth=cam.max_depth, samples=1, seed=seed,
                                            background=cam.background)
    assert not panics.any() and frame.any() and calls.min() >= 1 and calls.max() > 1
    assert np.array_equal(rgb.view(np.uint64), frame.view(np.uint64))
    # and a batch split in two with first_index is the same batch
    k = 1000
    lo = rq.oracle_radiance(drv, s, world, lights, rays[:k], max_depth=cam.max_depth, seed=seed, background=cam.background)
    hi = rq.oracle_radiance(drv, s, world, lights, rays[k:], max_depth=cam.max_depth, seed=seed, background=cam.background,
                            first_index=k)
    assert np.array_equal(np.concatenate([lo[0], hi[0]]).view(np.uint64), frame.view(np.uint64))


def test_driver_t_max_and_depth(rt):
    """One sphere under a sky: t_max cuts the first hit only, inclusive at the
    hit; depth 0 is black and no call."""
    drv = rq.driver(True)
    s = rt.Scene(drv)
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, -5.0), 1.0, s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))))
    sky = s.SkyGradient()
    rays = np.array([GOOD, GOOD[:7] + [3.9], GOOD[:7] + [4.0], GOOD[:7] + [float(np.nextafter(4.0, 0.0))],
                     [0, 0, 0, 0, 1, 0, 0, INF], [0, 0, 0, 0, 2, 0, 0, 0.5]], dtype=np.float64)
    # (each ray as a batch of its own: the same RNG pixel, so the same path where the first hit is the same)
    per = [rq.oracle_radiance(drv, s, w, None, r[None, :], background=sky, samples=1) for r in rays]
    rgb, calls, panics = (np.concatenate([p[k] for p in per]) for k in range(3))
    assert not panics.any()
    zenith = np.array([0.5, 0.7, 1.0])
    horizon_mix = 0.5 * np.array([1.0, 1.0, 1.0]) + 0.5 * zenith  # the sky at y = 0 (the ray along -z)
    np.testing.assert_allclose(rgb[1], horizon_mix, rtol=1e-15)
    np.testing.assert_array_equal(rgb[3], rgb[1])
    np.testing.assert_array_equal(rgb[2], rgb[0])       # t_max at the hit: the hit is taken
    assert list(calls[[1, 3, 4, 5]]) == [1, 1, 1, 1] and calls[0] >= 2 and calls[2] == calls[0]
    np.testing.assert_allclose(rgb[4], zenith, rtol=1e-15)
    np.testing.assert_array_equal(rgb[5], rgb[4])       # a miss is a miss under any t_max
    black = rq.oracle_radiance(drv, s, w, None, rays, background=sky, max_depth=0)
    assert not black[0].any() and not black[1].any() and not black[2].any()
    # four samples: the mean of four differently keyed paths, not four times the same
    r4 = rq.oracle_radiance(drv, s, w, None, rays[:1], background=sky, samples=4)
    assert r4[1][0] >= 4 * 2 and not np.array_equal(r4[0], rgb[:1])


# ---------------------------------------------------------------- the GPU test's ray sets
@pytest.mark.parametrize("name", sorted(rq.WORLDS))
def test_ray_sets_are_worth_the_query(product, capi, name):
    build, tier, lit = rq.WORLDS[name]
    rays, t = rq.world_rays(name)
    assert rays.shape == (rq.RAYS, 8)
    assert np.all(np.isfinite(rays[:, :7])) and np.all(rays[:, 7] > 0) and np.all(np.any(rays[:, 3:6] != 0, axis=1))
    length = np.linalg.norm(rays[:, 3:6], axis=1)
    assert length.min() < 1e-2 and length.max() > 1e2 and np.all((rays[:, 6] >= 0) & (rays[:, 6] < 1))
    finite = np.isfinite(rays[:, 7])
    assert finite.sum() == rq.RAYS // 10
    stats = []
    for samples, depth in ((1, rq.DEPTH), (4, rq.DEPTH), (1, 1), (4, 1)):
        cr = rq.reference(name, samples, depth, True)
        gl = rq.reference(name, samples, depth, False)
        # zero panics, on either build
        assert not cr[2].any() and not gl[2].any()
        assert np.isfinite(cr[0]).all()
        # glibc's libm against the correctly rounded functions: the rays the two disagree on
        off = 1.0 - rq.within(gl[0], cr[0]).mean()
        stats.append(off)
        assert off <= 1e-3, (samples, depth, off)
        assert (gl[1] != cr[1]).mean() <= 1e-3
        assert cr[1].max() <= samples * depth and cr[1].min() >= samples
    rgb, calls, _ = rq.reference(name, 1, rq.DEPTH, True)
    rgb1, calls1, _ = rq.reference(name, 1, 1, True)
    miss = t < 0
    beyond = finite & ~miss & (t > rays[:, 7])
    inside = finite & ~miss & (t <= rays[:, 7])
    lit_ends = ~miss & ~beyond & (rgb1.sum(axis=1) > 0)  # depth 1, a hit: what is left is the surface's emission
    print(f"{name}: miss {miss.mean():.3f}, >= 2 vertices {np.mean(calls >= 2):.3f}, first hit emits {int(lit_ends.sum())}, "
          f"t_max before the hit {int(beyond.sum())} / behind it {int(inside.sum())}, builds disagree {stats}")
    assert np.mean(calls >= 2) >= 0.25
    assert miss.sum() >= 20 and (~miss).sum() >= 20
    assert beyond.sum() >= 5 and inside.sum() >= 5
    assert np.all(calls[beyond | miss] == 1)
    if lit:
        assert lit_ends.sum() >= 5
    # the product's view of the same world: the tier it selects (host only)
    s, w, l, cam, _ = rq.world_case(product, name)
    info = capi.RtWorldInfo()
    bg = -1 if cam.background is None else cam.background.h
    product.check(product.world_info_get(s.s, w.h, -1 if l is None else l.h, bg, 0, C.byref(info)))
    assert info.kernel_tier == tier, info.kernel_tier
