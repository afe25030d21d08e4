"""rt_world_scatter without a device: the argument checks of the product's two
entry points and the structures' layout; and the oracle's scatter driver
(tests/cpp/scatter_oracle.cpp) pinned to the oracle proper -- iterated at
vertex 1..8 with stable indices and folded from the tail it must give
Camera::ray_color's radiance bit for bit on every ray of every world of
tests/radiance_query.py -- and to closed forms on single materials.
"""
import ctypes as C
import math

import numpy as np
import pytest

import radiance_query as rq
import scatter_query as sq

INF = float("inf")
EINVAL, EHANDLE, EMOVED, EDEVICE = -1, -2, -3, -7
GOOD = [0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, INF]


# ---------------------------------------------------------------- layout and defaults
def test_structures_have_the_abi_layout(product, capi, rt):
    assert C.sizeof(capi.RtScatterOpts) == 48
    assert [getattr(capi.RtScatterOpts, k).offset for k in
            ("struct_size", "flags", "seed", "sample", "vertex", "first_index", "background_tex", "stream",
             "reserved1")] == [0, 4, 8, 16, 20, 24, 28, 32, 40]
    assert C.sizeof(capi.RtScatter) == 224 and rt.SCATTER_DTYPE.itemsize == 224
    names = ("hit", "emitted", "f", "pdf", "origin", "dir", "eval_f", "eval_pdf", "flags", "draws")
    want = [0, 80, 104, 128, 136, 160, 184, 208, 216, 220]
    assert [getattr(capi.RtScatter, k).offset for k in names] == want
    assert [rt.SCATTER_DTYPE.fields[k][1] for k in names] == want
    assert rt.SCATTER_DTYPE.fields["hit"][0] == rt.HIT_DTYPE
    assert (capi.SCATTER_RAY, capi.SCATTER_PDF, capi.SCATTER_NO_SAMPLE, capi.SCATTER_EVAL, capi.SCATTER_PANIC) == \
        (1, 2, 4, 8, 16)
    o = capi.RtScatterOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    product.scatter_opts_default(C.byref(o))
    assert (o.struct_size, o.flags, o.seed, o.sample, o.vertex, o.first_index, o.background_tex, o.stream,
            o.reserved1) == (48, 0, 0, 0, 1, 0, -1, None, 0)
    product.scatter_opts_default(None)  # ignored


# ---------------------------------------------------------------- argument checks
def _one_sphere(rt, api):
    s = rt.Scene(api)
    m = s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))
    w = s.Hittables()
    w.add(s.Sphere((0.0, 0.0, -5.0), 1.0, m))
    return s, w


def _opts(product, capi, **over):
    o = capi.RtScatterOpts()
    product.scatter_opts_default(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


def _host(product, capi, s, world_h, rays, lights_h=-1, n=None, out=True, opts=True, eval_dirs=None, indices=None,
          **over):
    a = np.ascontiguousarray(rays, dtype=np.float64).reshape(-1, 8)
    n = len(a) if n is None else n
    rec = (capi.RtScatter * max(len(a), 1))()
    o = _opts(product, capi, **over)
    e = None if eval_dirs is None else np.ascontiguousarray(eval_dirs, dtype=np.float64)
    i = None if indices is None else np.ascontiguousarray(indices, dtype=np.uint32)
    return product.world_scatter(s.s if s is not None else None, world_h, lights_h, C.byref(o) if opts else None,
                                 a.ctypes.data_as(C.POINTER(capi.RtRay)),
                                 None if e is None else e.ctypes.data_as(C.POINTER(C.c_double)),
                                 None if i is None else i.ctypes.data_as(C.POINTER(C.c_uint32)), n,
                                 rec if out else None)


def _device(product, capi, s, world_h, lights_h=-1, n=1, rays=64, out=64, opts=True, indices=0, **over):
    """The device variant with made-up addresses: every check here comes before a device is touched."""
    o = _opts(product, capi, **over)
    return product.world_scatter_device(s.s if s is not None else None, world_h, lights_h,
                                        C.byref(o) if opts else None, C.c_void_p(rays) if rays else None, None,
                                        C.c_void_p(indices) if indices else None, n, C.c_void_p(out) if out else None)


def test_argument_checks(product, rt, capi):
    s, w = _one_sphere(rt, product)
    # n == 0: RT_OK, no device touched, no arrays needed -- in both variants
    o = _opts(product, capi)
    assert product.world_scatter(s.s, w.h, -1, C.byref(o), None, None, None, 0, None) == 0
    assert product.world_scatter_device(s.s, w.h, -1, C.byref(o), None, None, None, 0, None) == 0
    o = _opts(product, capi, flags=1, vertex=(1 << 28) - 1)  # RT_FLAG_REFERENCE_BVH, the last vertex
    assert product.world_scatter(s.s, w.h, -1, C.byref(o), None, None, None, 0, None) == 0
    # null scene, options or arrays
    assert _host(product, capi, None, w.h, [GOOD]) == EINVAL
    assert _host(product, capi, s, w.h, [GOOD], opts=False) == EINVAL
    assert _host(product, capi, s, w.h, [GOOD], out=False) == EINVAL
    o = _opts(product, capi)
    assert product.world_scatter(s.s, w.h, -1, C.byref(o), None, None, None, 1, (capi.RtScatter * 1)()) == EINVAL
    assert _device(product, capi, None, w.h) == EINVAL
    assert _device(product, capi, s, w.h, opts=False) == EINVAL
    assert _device(product, capi, s, w.h, rays=0) == EINVAL
    assert _device(product, capi, s, w.h, out=0) == EINVAL
    # struct_size below this version's (options not made by rt_scatter_opts_default)
    for size in (0, 47):
        assert _host(product, capi, s, w.h, [GOOD], struct_size=size) == EINVAL
        assert b"struct_size" in product.last_error()
        assert _device(product, capi, s, w.h, struct_size=size) == EINVAL
    assert _host(product, capi, s, w.h, [], n=0, struct_size=0) == EINVAL  # checked before n == 0 returns
    # flags other than RT_FLAG_REFERENCE_BVH
    for bad in (2, 3, 0x80000000):
        assert _host(product, capi, s, w.h, [GOOD], flags=bad) == EINVAL
        assert _device(product, capi, s, w.h, flags=bad) == EINVAL
    # a vertex outside [1, 2^28)
    for bad in (0, 1 << 28, 0xFFFFFFFF):
        assert _host(product, capi, s, w.h, [GOOD], vertex=bad) == EINVAL
        assert b"vertex" in product.last_error()
        assert _device(product, capi, s, w.h, vertex=bad) == EINVAL
    # first_index + n > 2^32 without indices (refused before an array is read); n >= 2^32 with or without
    assert _host(product, capi, s, w.h, [GOOD], n=2, first_index=0xFFFFFFFF) == EINVAL
    assert b"2^32" in product.last_error()
    assert _device(product, capi, s, w.h, n=2, first_index=0xFFFFFFFF) == EINVAL
    assert _device(product, capi, s, w.h, n=0, first_index=0xFFFFFFFF) == 0
    assert _host(product, capi, s, w.h, [GOOD], n=1 << 32) == EINVAL
    assert _device(product, capi, s, w.h, n=1 << 32) == EINVAL
    assert _device(product, capi, s, w.h, n=1 << 32, indices=64) == EINVAL
    # the device variant's records are written 16 B at a time
    for bad in (8, 72, 65):
        assert _device(product, capi, s, w.h, out=bad) == EINVAL
        assert b"16-B" in product.last_error()
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


@pytest.mark.parametrize("bad", [(0.0, 0.0, -0.0), (math.nan, 0.0, 1.0), (0.0, INF, 1.0), (1.0, 0.0, -INF)])
def test_host_variant_refuses_a_bad_eval_direction(product, rt, capi, bad):
    s, w = _one_sphere(rt, product)
    dirs = [(0.0, 1.0, 0.0), (0.0, 1.0, 0.0), bad]
    assert _host(product, capi, s, w.h, [GOOD, GOOD, GOOD], eval_dirs=dirs) == EINVAL
    assert b"eval direction 2" in product.last_error()
    # (a zero direction among the rays is named as a ray)
    assert _host(product, capi, s, w.h, [GOOD, [1.0, 2.0, 3.0, 0.0, -0.0, 0.0, 0.0, INF]]) == EINVAL
    assert b"ray 1" in product.last_error()


def test_wrong_shapes_raise(product, rt):
    s, w = _one_sphere(rt, product)
    for bad in (np.zeros(8), np.zeros((3, 7)), np.zeros((2, 3, 8))):
        with pytest.raises(ValueError, match=r"\(n, 8\)"):
            s.scatter(w, None, bad)
    with pytest.raises(ValueError, match="eval_dirs"):
        s.scatter(w, None, np.zeros((2, 8)), eval_dirs=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="indices"):
        s.scatter(w, None, np.zeros((2, 8)), indices=np.zeros(3, dtype=np.uint32))
    out = s.scatter(w, None, np.zeros((0, 8)))  # n == 0 needs no device
    assert out.shape == (0,) and out.dtype == rt.SCATTER_DTYPE


def test_no_device_is_an_error_not_a_fallback(product, rt, capi):
    """n > 0 needs a gfx950 device: RT_EDEVICE without one, never a CPU answer."""
    import torch
    s, w = _one_sphere(rt, product)
    rc = _host(product, capi, s, w.h, [GOOD])
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc == EDEVICE, product.last_error()
        assert _device(product, capi, s, w.h) == EDEVICE


# ---------------------------------------------------------------- the driver is ray_color
def _fold(levels):
    """ray_color's value from the records of its levels (camera.rs:286-325):
    `levels` = [(indices of the level's rays, records)], vertex 1 first; the
    depth below the last level returns BLACK."""
    n = len(levels[0][0])
    L = np.zeros((n, 3))
    for idx, rec in reversed(levels):
        below = L[idx]
        here = rec["emitted"].copy()  # a miss, None: the emission alone
        pdf = (rec["flags"] & sq.PDF) != 0
        sampled = pdf & ((rec["flags"] & sq.NO_SAMPLE) == 0)
        ray = (rec["flags"] & sq.RAY) != 0
        # color_from_emission + (albedo_x_pscatter * sample_color) / pdf_value; Vec3 / f64 = (1.0 / s) * v
        with np.errstate(all="ignore"):
            scat = (1.0 / rec["pdf"][sampled])[:, None] * (rec["f"][sampled] * below[sampled])
        here[sampled] = rec["emitted"][sampled] + scat
        # generate() returned None: color_from_emission + Color::default()
        none = pdf & ~sampled
        here[none] = rec["emitted"][none] + 0.0
        here[ray] = rec["emitted"][ray] + rec["f"][ray] * below[ray]
        L = np.zeros((n, 3))
        L[idx] = here
    return L


def _walk_levels(api, scene, world, rays, background, depth):
    """orcx_world_scatter at vertex 1..depth with stable indices, following
    (origin, dir), the time kept, t_max = inf after the first."""
    idx = np.arange(len(rays), dtype=np.uint32)
    cur = np.array(rays)
    levels = []
    for k in range(1, depth + 1):
        rec = sq.oracle_scatter(api, scene, world, cur, indices=idx, vertex=k, background=background)
        levels.append((idx, rec))
        go = ((rec["flags"] & sq.RAY) != 0) | ((rec["flags"] & (sq.PDF | sq.NO_SAMPLE)) == sq.PDF)
        nxt = np.zeros((int(go.sum()), 8))
        nxt[:, 0:3] = rec["origin"][go]
        nxt[:, 3:6] = rec["dir"][go]
        nxt[:, 6] = cur[go, 6]
        nxt[:, 7] = np.inf
        idx, cur = idx[go], nxt
        if not len(idx):
            break
    return levels


@pytest.mark.parametrize("name", list(rq.WORLDS))
def test_driver_iterated_is_ray_color(name):
    """lights = None: the levels of orcx_world_scatter folded from the tail are
    orcx_world_radiance, to the last bit of every f64 on every ray, at depth 8
    and at depth 1; no level and no ray_color panics, so no ray is left out."""
    drv = sq.driver(True)
    s, world, _, cam, _ = sq.oracle_world(name, True)
    rays, _ = rq.world_rays(name)
    for depth in (rq.DEPTH, 1):
        levels = _walk_levels(drv, s, world, rays, cam.background, depth)
        for k, (_, rec) in enumerate(levels):
            assert not (rec["flags"] & sq.PANIC).any(), (depth, k + 1)
            sampled = (rec["flags"] & (sq.PDF | sq.NO_SAMPLE)) == sq.PDF
            assert np.all(rec["pdf"][sampled] != 0.0)  # ray_color's assert (camera.rs:309) holds on every ray
        L = _fold(levels)
        rgb, calls, panics = rq.oracle_radiance(drv, s, world, None, rays, max_depth=depth, samples=1,
                                                background=cam.background)
        assert not panics.any()
        assert np.isfinite(L).all()
        differ = np.nonzero((sq.bits(L) != sq.bits(rgb)).any(axis=1))[0]
        print(f"{name} depth {depth}: {len(levels)} levels, rays a level {[len(i) for i, _ in levels]}, "
              f"rays that differ {len(differ)}")
        for i in differ[:5]:
            print(f"  ray {i}: folded {L[i]} ray_color {rgb[i]}")
        assert not len(differ)
        # one ray_color call per level a ray reached
        reached = np.zeros(len(rays), dtype=np.uint32)
        for idx, _ in levels:
            reached[idx] += 1
        assert np.array_equal(reached, calls)
        # at depth 8 the fold is not of one level only: a quarter of the rays go on (tests/test_world_radiance_cpu.py)
        assert len(levels) == 1 if depth == 1 else len(levels[1][0]) >= len(rays) // 4


# ---------------------------------------------------------------- closed forms
def _rays_at(target, origins):
    o = np.asarray(origins, dtype=np.float64)
    r = np.zeros((len(o), 8))
    r[:, 0:3] = o
    r[:, 3:6] = np.asarray(target, dtype=np.float64) - o
    r[:, 7] = np.inf
    return r


def _scene(rt, mat_of, medium=False):
    """A unit quad in the plane y = 0 (normal +y from above) of mat_of(scene)."""
    drv = sq.driver(True)
    s = rt.Scene(drv)
    w = s.Hittables()
    q = s.Quad((-1.0, 0.0, -1.0), (0.0, 0.0, 2.0), (2.0, 0.0, 0.0), mat_of(s))
    w.add(q)
    return drv, s, w


ORIGINS = [(0.3, 2.0, 0.1), (-0.7, 0.5, 0.4), (0.2, 1.0, -3.0), (2.0, 0.25, 2.0)]
TARGET = (0.1, 0.0, -0.2)


def test_lambertian_quad_closed_form(rt):
    albedo = np.array([0.8, 0.4, 0.2])
    drv, s, w = _scene(rt, lambda s: s.Lambertian(s.SolidColor(tuple(albedo))))
    rays = _rays_at(TARGET, ORIGINS)
    g = np.random.default_rng(7)
    ev = g.standard_normal((len(rays), 3))
    ev[0] = (0.0, -1.0, 0.0)  # below the surface: f and pdf are 0
    rec = sq.oracle_scatter(drv, s, w, rays, eval_dirs=ev)
    assert np.all(rec["flags"] == sq.PDF | sq.EVAL) and np.all(rec["draws"] == 2)
    assert np.all(rec["hit"]["flags"] == 3) and np.all(rec["hit"]["normal"] == (0.0, 1.0, 0.0))
    assert not rec["emitted"].any()
    np.testing.assert_allclose(rec["origin"], rec["hit"]["p"], rtol=0, atol=0)
    for d, f, pdf in ((rec["dir"], rec["f"], rec["pdf"]), (ev, rec["eval_f"], rec["eval_pdf"])):
        cos = d[:, 1] / np.linalg.norm(d, axis=1)
        np.testing.assert_allclose(pdf, np.maximum(0.0, cos / math.pi), rtol=1e-14, atol=0)
        np.testing.assert_allclose(f, albedo[None, :] * np.maximum(cos, 0.0)[:, None] / math.pi, rtol=1e-14, atol=0)
    assert np.all(rec["pdf"] > 0) and np.all(rec["dir"][:, 1] > 0)
    assert rec["eval_pdf"][0] == 0.0 and not rec["eval_f"][0].any()
    # the direction made is evaluated again as an eval direction: the same bits
    again = sq.oracle_scatter(drv, s, w, rays, eval_dirs=rec["dir"])
    assert np.array_equal(sq.bits(again["eval_f"]), sq.bits(rec["f"]))
    assert np.array_equal(sq.bits(again["eval_pdf"]), sq.bits(rec["pdf"]))
    # a miss: the background, everything else zero
    sky = s.SkyGradient()
    miss = sq.oracle_scatter(drv, s, w, _rays_at((0.0, 5.0, 0.0), [(0.0, 1.0, 0.0)]), eval_dirs=[(0.0, 1.0, 0.0)],
                             background=sky)
    np.testing.assert_allclose(miss["emitted"][0], (0.5, 0.7, 1.0), rtol=1e-15)
    assert miss["flags"][0] == 0 and miss["draws"][0] == 0 and miss["hit"]["mat"][0] == -1 and miss["hit"]["flags"][0] == 0
    assert not miss["f"].any() and not miss["dir"].any() and not miss["eval_f"].any()
    # t_max before the quad: a miss as well
    cut = rays.copy()
    cut[:, 7] = 0.5
    assert not sq.oracle_scatter(drv, s, w, cut)["hit"]["flags"].any()


def test_medium_is_the_sphere_pdf(rt):
    drv = sq.driver(True)
    s = rt.Scene(drv)
    w = s.Hittables()
    w.add(s.ConstantMedium(s.Sphere((0.0, 0.0, 0.0), 1.0, s.EmptyMaterial()), 50.0, s.SolidColor((0.9, 0.6, 0.3))))
    rays = _rays_at((0.0, 0.0, 0.0), ORIGINS)
    rec = sq.oracle_scatter(drv, s, w, rays, eval_dirs=np.tile([[0.0, 0.0, 1.0]], (len(rays), 1)))
    found = (rec["hit"]["flags"] & 1) != 0
    assert found.sum() >= 3  # (the density makes a pass-through improbable, not impossible)
    r = rec[found]
    assert np.all(r["hit"]["flags"] & 4) and np.all(r["flags"] == sq.PDF | sq.EVAL) and np.all(r["draws"] == 2)
    assert np.all(r["pdf"] == 1.0 / (4.0 * math.pi)) and np.all(r["eval_pdf"] == 1.0 / (4.0 * math.pi))
    np.testing.assert_allclose(r["f"], np.tile(np.array([0.9, 0.6, 0.3]) / (4.0 * math.pi), (len(r), 1)), rtol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(r["dir"], axis=1), 1.0, rtol=1e-14)


@pytest.mark.parametrize("kind", ["metal", "dielectric", "transparent", "portal"])
def test_specular_materials_return_a_ray(rt, kind):
    off = (0.5, -2.0, 0.25)
    make = {"metal": lambda s: s.Metal((0.9, 0.8, 0.7), 0.05),
            "dielectric": lambda s: s.Dielectric(s.SolidColor((0.95, 0.9, 0.85)), 1.5),
            "transparent": lambda s: s.Transparent(),
            "portal": lambda s: s.Portal((0.5, 0.6, 0.7), offset=off)}[kind]
    drv, s, w = _scene(rt, make)
    rays = _rays_at(TARGET, ORIGINS)
    rec = sq.oracle_scatter(drv, s, w, rays, eval_dirs=np.tile([[0.0, 1.0, 0.0]], (len(rays), 1)))
    assert np.all(rec["flags"] == sq.RAY)  # no EVAL bit: there is no PDF to evaluate
    assert not rec["pdf"].any() and not rec["eval_f"].any() and not rec["eval_pdf"].any() and not rec["emitted"].any()
    assert list(rec["draws"]) == {"metal": [2] * 4, "transparent": [0] * 4, "portal": [0] * 4}.get(kind, list(rec["draws"]))
    want_f = {"metal": (0.9, 0.8, 0.7), "dielectric": (0.95, 0.9, 0.85), "transparent": (1.0, 1.0, 1.0),
              "portal": (0.5, 0.6, 0.7)}[kind]
    assert np.all(rec["f"] == want_f)
    if kind == "portal":
        np.testing.assert_array_equal(rec["origin"], rec["hit"]["p"] + np.array(off))
        np.testing.assert_array_equal(rec["dir"], rays[:, 3:6])  # the identity quaternion
    else:
        np.testing.assert_array_equal(rec["origin"], rec["hit"]["p"])
    if kind == "transparent":
        np.testing.assert_array_equal(rec["dir"], rays[:, 3:6])
    if kind == "dielectric":
        assert set(rec["draws"]) <= {0, 1} and (rec["draws"] == 1).any()
    if kind == "metal":
        assert np.all(rec["dir"][:, 1] > 0)


def test_a_bare_light_emits_and_does_not_scatter(rt):
    drv, s, w = _scene(rt, lambda s: s.DiffuseLight(s.SolidColor((4.0, 3.0, 2.0))))
    rays = _rays_at(TARGET, ORIGINS)
    rec = sq.oracle_scatter(drv, s, w, rays, eval_dirs=np.tile([[0.0, 1.0, 0.0]], (len(rays), 1)))
    assert np.all(rec["emitted"] == (4.0, 3.0, 2.0))
    assert not rec["flags"].any() and not rec["draws"].any()
    for k in ("f", "pdf", "origin", "dir", "eval_f", "eval_pdf"):
        assert not rec[k].any(), k
    assert np.all(rec["hit"]["flags"] & 1)
    # a light over a Lambertian scatters as the Lambertian, and a Mix draws first
    drv, s, w = _scene(rt, lambda s: s.Mix(s.DiffuseLight(s.SolidColor((4.0, 3.0, 2.0)),
                                                          s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))),
                                           s.Metal((0.9, 0.9, 0.9), 0.0), 0.5))
    many = np.tile(rays, (8, 1))
    rec = sq.oracle_scatter(drv, s, w, many)
    assert np.all(rec["emitted"] == (2.0, 1.5, 1.0))  # mat1 * (1 - r) + mat2 * r
    assert set(rec["flags"]) == {sq.RAY, sq.PDF} and np.all(rec["draws"] == 3)
