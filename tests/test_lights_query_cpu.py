"""rt_lights_pdf / rt_lights_sample without a device: the argument checks of
the product's four entry points, the structures' sizes and the Python mirror's
shapes; and the oracle's lights driver (tests/cpp/lights_oracle.cpp) against
closed forms evaluated in numpy, which is what makes the driver an independent
witness for tests/test_lights_query_gpu.py -- a quad's and a sphere's
pdf_value, every sampled direction hitting the lights, a list's uniform child
choice, the mean of 1 / pdf as the quad's solid angle -- and the sample
driver's RNG keying.
"""
import ctypes as C
import math

import numpy as np
import pytest

import lights_query as lq

INF = float("inf")
EINVAL, EHANDLE, EMOVED, EPANIC, EUNSUPPORTED, EDEVICE = -1, -2, -3, -5, -6, -7
_DP = C.POINTER(C.c_double)


def test_structures_have_the_abi_sizes(product, capi, rt):
    assert C.sizeof(capi.RtLightsOpts) == 48
    assert C.sizeof(capi.RtLightSample) == 40 and rt.LIGHT_SAMPLE_DTYPE.itemsize == 40
    assert [rt.LIGHT_SAMPLE_DTYPE.fields[k][1] for k in ("dir", "pdf", "flags", "reserved")] == [0, 24, 32, 36]
    assert [getattr(capi.RtLightsOpts, k).offset for k in ("struct_size", "flags", "seed", "samples", "first_index",
                                                            "background_tex", "reserved", "stream", "reserved1")] == \
        [0, 4, 8, 16, 20, 24, 28, 32, 40]
    o = capi.RtLightsOpts()
    C.memset(C.byref(o), 0xFF, C.sizeof(o))
    product.lights_opts_default(C.byref(o))
    assert (o.struct_size, o.flags, o.seed, o.samples, o.first_index, o.background_tex, o.reserved, o.stream,
            o.reserved1) == (48, 0, 0, 1, 0, -1, 0, None, 0)
    product.lights_opts_default(None)  # ignored
    assert capi.LIGHT_PANIC == 1


def _scene(rt, api):
    """A floor and, as lights, one quad."""
    s = rt.Scene(api)
    w = s.Hittables()
    w.add(s.Quad((-5.0, 0.0, -5.0), (10.0, 0.0, 0.0), (0.0, 0.0, 10.0), s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))))
    l = s.Quad((-0.5, 2.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), s.DiffuseLight(s.SolidColor((4.0, 4.0, 4.0))))
    return s, w, l


def _opts(product, capi, **over):
    o = capi.RtLightsOpts()
    product.lights_opts_default(C.byref(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


GOOD_O, GOOD_D = [0.0, 0.5, 0.0], [0.0, 1.0, 0.0]


def _pdf(product, capi, s, wh, lh, origins=(GOOD_O,), dirs=(GOOD_D,), n=None, opts=True, out=True, **over):
    o_ = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d_ = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = len(o_) if n is None else n
    res = (C.c_double * max(len(o_), 1))()
    o = _opts(product, capi, **over)
    return product.lights_pdf(s.s if s is not None else None, wh, lh, C.byref(o) if opts else None,
                              o_.ctypes.data_as(_DP), d_.ctypes.data_as(_DP), n, res if out else None)


def _sample(product, capi, s, wh, lh, origins=(GOOD_O,), n=None, opts=True, out=True, **over):
    o_ = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    n = len(o_) if n is None else n
    o = _opts(product, capi, **over)
    res = (capi.RtLightSample * max(len(o_) * max(o.samples, 1), 1))()
    return product.lights_sample(s.s if s is not None else None, wh, lh, C.byref(o) if opts else None,
                                 o_.ctypes.data_as(_DP), n, res if out else None)


def _pdf_dev(product, capi, s, wh, lh, n=1, origins=64, dirs=64, out=64, opts=True, **over):
    """The device variants with made-up addresses: every check here comes before a device is touched."""
    o = _opts(product, capi, **over)
    return product.lights_pdf_device(s.s if s is not None else None, wh, lh, C.byref(o) if opts else None,
                                     C.c_void_p(origins) if origins else None, C.c_void_p(dirs) if dirs else None, n,
                                     C.c_void_p(out) if out else None)


def _sample_dev(product, capi, s, wh, lh, n=1, origins=64, out=64, opts=True, **over):
    o = _opts(product, capi, **over)
    return product.lights_sample_device(s.s if s is not None else None, wh, lh, C.byref(o) if opts else None,
                                        C.c_void_p(origins) if origins else None, n, C.c_void_p(out) if out else None)


ALL = (_pdf, _sample, _pdf_dev, _sample_dev)


def test_argument_checks(product, rt, capi):
    s, w, l = _scene(rt, product)
    # n == 0: RT_OK, no device touched, no arrays needed -- in all four variants
    o = _opts(product, capi, flags=1)
    assert product.lights_pdf(s.s, w.h, l.h, C.byref(o), None, None, 0, None) == 0
    assert product.lights_pdf_device(s.s, w.h, l.h, C.byref(o), None, None, 0, None) == 0
    assert product.lights_sample(s.s, w.h, l.h, C.byref(o), None, 0, None) == 0
    assert product.lights_sample_device(s.s, w.h, l.h, C.byref(o), None, 0, None) == 0
    for f in ALL:
        # null scene or options
        assert f(product, capi, None, w.h, l.h) == EINVAL
        assert f(product, capi, s, w.h, l.h, opts=False) == EINVAL
        # null arrays
        assert f(product, capi, s, w.h, l.h, out=False) == EINVAL
        # struct_size below this version's
        for size in (0, 47):
            assert f(product, capi, s, w.h, l.h, struct_size=size) == EINVAL
            assert b"struct_size" in product.last_error()
        assert f(product, capi, s, w.h, l.h, n=0, struct_size=0) == EINVAL  # checked before n == 0 returns
        # flags other than RT_FLAG_REFERENCE_BVH
        for bad in (2, 3, 0x80000000):
            assert f(product, capi, s, w.h, l.h, flags=bad) == EINVAL
        # first_index + n > 2^32 (refused before an array is read); exactly 2^32 passes this check
        assert f(product, capi, s, w.h, l.h, n=(1 << 32) + 1) == EINVAL
        assert b"2^32" in product.last_error()
        assert f(product, capi, s, w.h, l.h, n=2, first_index=0xFFFFFFFF) == EINVAL
        assert f(product, capi, s, w.h, l.h, n=0, first_index=0xFFFFFFFF) == 0
        # lights = -1: `lights: None` has nothing to sample
        assert f(product, capi, s, w.h, -1) == EINVAL
        assert b"lights" in product.last_error()
        # handles
        for h in (-1, 9999):
            assert f(product, capi, s, h, l.h) == EHANDLE
        for h in (-2, 9999):
            assert f(product, capi, s, w.h, h) == EHANDLE
            assert f(product, capi, s, w.h, l.h, background_tex=h) == EHANDLE
    assert _pdf_dev(product, capi, s, w.h, l.h, origins=0) == EINVAL
    assert _pdf_dev(product, capi, s, w.h, l.h, dirs=0) == EINVAL
    assert _sample_dev(product, capi, s, w.h, l.h, origins=0) == EINVAL
    assert product.lights_pdf(s.s, w.h, l.h, C.byref(_opts(product, capi)), None, None, 1, (C.c_double * 1)()) == EINVAL
    # samples == 0: the sample query only (the pdf query ignores the field)
    assert _sample(product, capi, s, w.h, l.h, samples=0) == EINVAL
    assert b"samples" in product.last_error()
    assert _sample_dev(product, capi, s, w.h, l.h, samples=0) == EINVAL
    assert _pdf_dev(product, capi, s, w.h, l.h, n=0, samples=0) == 0
    # n * samples >= 2^40 (the sample query only)
    assert _sample_dev(product, capi, s, w.h, l.h, n=1 << 20, samples=1 << 20) == EINVAL
    assert b"2^40" in product.last_error()
    assert _sample_dev(product, capi, s, w.h, l.h, n=1 << 32, samples=256) == EINVAL
    assert _sample(product, capi, s, w.h, l.h, n=1 << 30, samples=1 << 10) == EINVAL
    assert _sample_dev(product, capi, s, w.h, l.h, n=0, samples=0xFFFFFFFF) == 0
    # a handle moved into another object
    outer = s.Hittables()
    outer.add(w)
    for f in ALL:
        assert f(product, capi, s, w.h, l.h) == EMOVED
    ll = s.Hittables()
    ll.add(l)
    for f in ALL:
        assert f(product, capi, s, outer.h, l.h) == EMOVED


@pytest.mark.parametrize("which, field, value", [("origin", 0, math.nan), ("origin", 1, INF), ("origin", 2, -INF),
                                                 ("direction", 0, math.nan), ("direction", 1, INF),
                                                 ("direction", 2, -INF)])
def test_host_variants_refuse_a_bad_point(product, rt, capi, which, field, value):
    s, w, l = _scene(rt, product)
    origins, dirs = [list(GOOD_O) for _ in range(3)], [list(GOOD_D) for _ in range(3)]
    (origins if which == "origin" else dirs)[1][field] = value
    assert _pdf(product, capi, s, w.h, l.h, origins, dirs) == EINVAL
    assert (which + " 1").encode() in product.last_error()
    if which == "origin":
        assert _sample(product, capi, s, w.h, l.h, origins) == EINVAL
        assert b"origin 1" in product.last_error()


def test_host_pdf_refuses_a_zero_direction(product, rt, capi):
    s, w, l = _scene(rt, product)
    assert _pdf(product, capi, s, w.h, l.h, [GOOD_O, GOOD_O], [GOOD_D, [0.0, -0.0, 0.0]]) == EINVAL
    assert b"direction 1" in product.last_error()


def _refused_lights(rt, s):
    """name -> (lights object, rt_render's code): what a lights object may not be."""
    m = s.DiffuseLight(s.SolidColor((4.0, 4.0, 4.0)))
    inner = s.Hittables()
    inner.add(s.Sphere((0.0, 2.0, 0.0), 0.5, m))
    with_bvh = s.Hittables()
    with_bvh.add(s.Quad((-0.5, 3.0, -0.5), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), m))
    with_bvh.add(s.BVH(inner))
    with_medium = s.Hittables()
    with_medium.add(s.ConstantMedium(s.Sphere((0.0, 2.0, 0.0), 0.5, m), 0.1, s.SolidColor((1.0, 1.0, 1.0))))
    deep = s.Sphere((0.0, 2.0, 0.0), 0.5, m)
    for _ in range(5):  # five list levels over the sphere
        outer = s.Hittables()
        outer.add(deep)
        deep = outer
    ok4 = s.Sphere((0.0, 2.0, 0.0), 0.5, m)
    for _ in range(4):
        outer = s.Hittables()
        outer.add(ok4)
        ok4 = outer
    return {"bvh": (with_bvh, EPANIC), "medium": (with_medium, EPANIC), "empty": (s.Hittables(), EPANIC),
            "depth5": (deep, EUNSUPPORTED), "depth4": (ok4, None)}


def test_lights_rt_render_refuses_are_refused_with_its_code_and_message(product, rt, capi):
    """A BVH or a ConstantMedium among the lights, an empty list, a tree of
    five levels: rt_render's code and message (its flattening's, which
    rt_world_info_get reports without a device), from all four variants, before
    a device is touched; four levels pass these checks."""
    import torch
    s, w, _ = _scene(rt, product)
    for name, (l, code) in _refused_lights(rt, s).items():
        info = capi.RtWorldInfo()
        rc = product.world_info_get(s.s, w.h, l.h, -1, 0, C.byref(info))
        if code is None:
            assert rc == 0, (name, product.last_error())
            want = 0 if torch.cuda.is_available() else EDEVICE
            assert _pdf(product, capi, s, w.h, l.h, [[0.0, 0.5, 0.0]], [[0.0, 1.0, 0.0]]) == want
            continue
        assert rc == code, (name, rc, product.last_error())
        msg = product.last_error()
        assert msg
        for f in ALL:
            assert f(product, capi, s, w.h, l.h) == code, (name, f.__name__)
            assert product.last_error() == msg, (name, f.__name__)
    assert b"BVH" in _msg(product, capi, rt, "bvh") and b"ConstantMedium" in _msg(product, capi, rt, "medium")
    assert b"empty" in _msg(product, capi, rt, "empty") and b"deeper than 4" in _msg(product, capi, rt, "depth5")


def _msg(product, capi, rt, name):
    s, w, _ = _scene(rt, product)
    l, code = _refused_lights(rt, s)[name]
    assert _sample_dev(product, capi, s, w.h, l.h) == code
    return product.last_error()


def test_the_mirror_checks_shapes_and_returns_the_documented_ones(product, rt):
    s, w, l = _scene(rt, product)
    for bad in (np.zeros(3), np.zeros((3, 2)), np.zeros((2, 3, 3))):
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            s.lights_pdf(w, l, bad, bad)
        with pytest.raises(ValueError, match=r"\(n, 3\)"):
            s.lights_sample(w, l, bad)
    with pytest.raises(ValueError, match="same shape"):
        s.lights_pdf(w, l, np.zeros((2, 3)), np.ones((3, 3)))
    # n == 0 needs no device
    p = s.lights_pdf(w, l, np.zeros((0, 3)), np.zeros((0, 3)))
    assert p.shape == (0,) and p.dtype == np.float64
    q = s.lights_sample(w, l, np.zeros((0, 3)), samples=3, seed=9, first_index=5)
    assert q.shape == (0, 3) and q.dtype == rt.LIGHT_SAMPLE_DTYPE
    with pytest.raises(rt.RtError, match="samples"):
        s.lights_sample(w, l, np.zeros((0, 3)), samples=0)


def test_no_device_is_an_error_not_a_fallback(product, rt, capi):
    """n > 0 needs a gfx950 device: RT_EDEVICE without one, never a CPU answer."""
    import torch
    s, w, l = _scene(rt, product)
    rc = _pdf(product, capi, s, w.h, l.h)
    if torch.cuda.is_available():
        assert rc == 0
    else:
        assert rc == EDEVICE, product.last_error()
        assert _sample(product, capi, s, w.h, l.h) == EDEVICE
        assert _pdf_dev(product, capi, s, w.h, l.h) == EDEVICE
        assert _sample_dev(product, capi, s, w.h, l.h) == EDEVICE


# ---------------------------------------------------------------- the driver against closed forms
def test_driver_quad_pdf_is_the_closed_form(rt):
    """The unit quad of `one_quad` from points on its axis, towards points of
    it: pdf = d^2 / (cos * area) (quad.rs:108-120), in numpy; the direction's
    length does not matter, a direction past the quad gives 0."""
    drv = lq.driver()
    s, w, l, _ = lq.oracle_case("one_quad")
    g = np.random.default_rng(1)
    n = 500
    h = g.uniform(0.05, 30.0, size=n)
    o = np.stack([np.zeros(n), 2.0 - h, np.zeros(n)], axis=1)
    p = np.stack([g.uniform(-0.5, 0.5, n), np.full(n, 2.0), g.uniform(-0.5, 0.5, n)], axis=1)
    d = (p - o) * g.uniform(0.01, 100.0, size=(n, 1))
    dist2 = np.sum((p - o) ** 2, axis=1)
    cos = h / np.sqrt(dist2)
    got = lq.oracle_pdf(drv, s, l, o, d)
    np.testing.assert_allclose(got, dist2 / (cos * 1.0), rtol=1e-12)
    away = np.stack([g.uniform(0.6, 3.0, n), np.full(n, 2.0), g.uniform(0.6, 3.0, n)], axis=1) - o
    assert not lq.oracle_pdf(drv, s, l, o, away).any()
    assert not lq.oracle_pdf(drv, s, l, o, -d).any()  # behind the origin: outside [1e-8, inf)


def test_driver_sphere_pdf_is_the_closed_form(rt):
    """1 / (2 pi (1 - sqrt(1 - r^2 / d^2))) towards the sphere from outside
    (sphere.rs:114-132), 1 / 4 pi from inside, 0 past it."""
    drv = lq.driver()
    s, w, l, _ = lq.oracle_case("one_sphere")
    c, r = np.array(lq.SPHERE[0]), lq.SPHERE[1]
    g = np.random.default_rng(2)
    n = 500
    dist = r * 10.0 ** g.uniform(0.01, 3.0, size=(n, 1))
    o = c + lq._isotropic(g, n) * dist
    d = (c - o) * g.uniform(0.01, 100.0, size=(n, 1))
    want = 1.0 / (2.0 * np.pi * (1.0 - np.sqrt(1.0 - r * r / dist[:, 0] ** 2)))
    # (1 - sqrt(1 - x) loses digits as x -> 0: a relative 1e-16 of 1 is 1e-16 / (x / 2) of the result; x >= 1e-6 here)
    np.testing.assert_allclose(lq.oracle_pdf(drv, s, l, o, d), want, rtol=1e-9)
    assert not lq.oracle_pdf(drv, s, l, o, -d).any()
    inside = c + lq._isotropic(g, n) * r * g.uniform(0.0, 0.95, size=(n, 1))
    assert np.all(lq.oracle_pdf(drv, s, l, inside, lq._isotropic(g, n)) == 1.0 / (4.0 * np.pi))


@pytest.mark.parametrize("name", sorted(lq.SETS))
def test_driver_every_sampled_direction_hits_the_lights(name):
    """... and is a unit vector with a positive finite pdf; a panicked draw is zeros and the flag."""
    drv = lq.driver()
    s, w, l, _ = lq.oracle_case(name)
    o, d, pdf, smp = lq.reference(name)
    good = smp["flags"] == 0
    assert set(np.unique(smp["flags"])) <= {0, lq.PANIC}
    bad = smp[~good]
    assert not bad["dir"].any() and not bad["pdf"].any()
    og = np.repeat(o, lq.SAMPLES, axis=0)[good.reshape(-1)]
    leaf = lq.oracle_leaf(drv, s, l, og, smp["dir"][good])
    print(f"{name}: {good.sum()} good draws, {(~good).sum()} panicked, leaves {np.unique(leaf, return_counts=True)}")
    assert np.all(leaf >= 0)
    np.testing.assert_allclose(np.linalg.norm(smp["dir"][good], axis=1), 1.0, rtol=1e-14)
    assert np.all(np.isfinite(smp["pdf"][good])) and np.all(smp["pdf"][good] > 0)
    # the driver's two entry points agree with each other
    assert lq.same_bits(lq.oracle_pdf(drv, s, l, og, smp["dir"][good]), smp["pdf"][good])
    assert pdf.shape == (lq.N,) and np.all(np.isfinite(d)) and np.all(np.any(d != 0, axis=1))
    length = np.linalg.norm(d, axis=1)
    assert length.min() < 1e-2 and length.max() > 1e2


def test_driver_flat_list_chooses_its_children_uniformly():
    """30 000 draws from round the origin, where no direction meets two of
    `flat`'s lights: each child's share is within 5 sigma of 1 / 3
    (hits.rs:69-75)."""
    drv = lq.driver()
    s, w, l, _ = lq.oracle_case("flat")
    g = np.random.default_rng(3)
    n, k = 100, 300
    o = np.array([0.0, 0.5, 0.0]) + g.uniform(-0.2, 0.2, size=(n, 3))
    smp = lq.oracle_sample(drv, s, l, o, k, seed=11)
    assert not smp["flags"].any()
    leaf = lq.oracle_leaf(drv, s, l, np.repeat(o, k, axis=0), smp["dir"].reshape(-1, 3))
    total = n * k
    sigma = math.sqrt(total * (1.0 / 3.0) * (2.0 / 3.0))
    counts = [int(np.sum(leaf == c)) for c in range(3)]
    print("child counts", counts, "sigma", sigma)
    assert sum(counts) == total
    for c in counts:
        assert abs(c - total / 3.0) <= 5.0 * sigma


def test_driver_mean_of_one_over_pdf_is_the_quads_solid_angle():
    """E[1 / pdf] over draws towards `one_quad` from a point is the quad's
    solid angle there: the integral of cos / d^2 over the quad, by the midpoint
    rule in numpy."""
    drv = lq.driver()
    s, w, l, _ = lq.oracle_case("one_quad")
    o = np.array([[0.7, 0.9, -0.4]])
    k = 30_000
    smp = lq.oracle_sample(drv, s, l, o, k, seed=13)[0]
    assert not smp["flags"].any()
    inv = 1.0 / smp["pdf"]
    mean, sem = inv.mean(), inv.std(ddof=1) / math.sqrt(k)
    m = 2000
    t = (np.arange(m) + 0.5) / m - 0.5
    x, z = np.meshgrid(t, t)
    v = np.stack([x - o[0, 0], np.full_like(x, 2.0 - o[0, 1]), z - o[0, 2]], axis=-1)
    d2 = np.sum(v * v, axis=-1)
    omega = float(np.sum((v[..., 1] / np.sqrt(d2)) / d2) / (m * m))  # (area 1; the normal is y)
    print(f"solid angle {omega:.6f}, mean 1 / pdf {mean:.6f} +- {sem:.6f}")
    assert abs(mean - omega) <= 5.0 * sem


def test_driver_sample_keying():
    """One origin at first_index 7 with 3 samples is three one-sample calls at
    sample 0, 1, 2 -- which the driver can only be asked for as the first,
    second and third of a 3-sample call, so: the same as the same origin at
    index 7 of a longer batch; another index, another sample or another seed is
    another draw."""
    drv = lq.driver()
    s, w, l, _ = lq.oracle_case("tree")
    o = np.array([[0.3, 0.8, -0.2]])
    three = lq.oracle_sample(drv, s, l, o, 3, seed=21, first_index=7)
    batch = lq.oracle_sample(drv, s, l, np.repeat(o, 9, axis=0), 3, seed=21, first_index=0)
    assert lq.same_samples(three, batch[7:8])
    for k in range(3):  # a call of k + 1 samples ends on sample k
        assert lq.same_samples(lq.oracle_sample(drv, s, l, o, k + 1, seed=21, first_index=7)[:, k], three[:, k])
    dirs = [tuple(x) for x in batch["dir"].reshape(-1, 3)]
    assert len(set(dirs)) == len(dirs)  # every (index, sample) its own draw
    other = lq.oracle_sample(drv, s, l, o, 3, seed=22, first_index=7)
    assert not np.array_equal(other["dir"], three["dir"])
