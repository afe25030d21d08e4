"""Shared by tests/test_edge_values_cpu.py and tests/test_edge_values_gpu.py:
Disney parameter sets at the values where disney.rs is singular or changes
branch, and texture-addressing probes at the values where texture.rs rounds,
clamps, wraps or casts, with an independent numpy model of texture.rs:59-73,
111-163 that writes Rust's cast semantics out (`as i32` / `as u32` / `as i64`
saturate, NaN -> 0, i32 addition wraps as in a release build).

Every comparison built on this module is on bit patterns, NaN equal to NaN.
"""
import ctypes as C
import functools
import math
import os
import tempfile

import numpy as np

from conftest import pkg_module
import disney_query as dq
import obj_disney_query as oq
import scatter_query as sq

F = np.float64


def nxt(x, up=True):
    return float(np.nextafter(F(x), F(np.inf if up else -np.inf)))


@functools.lru_cache(maxsize=None)
def driver():
    """The one oracle driver of these tests (tests/cpp/edge_oracle.cpp, built
    once per process as obj_disney_query builds its own, which this one
    includes): the loader with Disney materials, orcx_world_scatter,
    orcx_camera_rays, orcx_world_radiance, orcx_disney_selftest and
    orcx_render_partials_loop, bound as .x_*."""
    import subprocess
    from conftest import ROOT
    capi = pkg_module("capi")
    tmp = tempfile.TemporaryDirectory(prefix="edge_query_")
    _TMP.append(tmp)
    out = os.path.join(tmp.name, "libedge_oracle_cr.so")
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-DORC_CRMATH", "-shared", "-o", out,
           os.path.join(ROOT, "tests", "cpp", "edge_oracle.cpp"), os.path.join(ROOT, "oracle", "rt_oracle.cpp"),
           os.path.join(ROOT, "oracle", "rt_oracle_obj.cpp"), "-pthread", "-lz"]
    subprocess.run(cmd, check=True, timeout=600)
    lib = C.CDLL(out)
    api = capi.Api(lib, "orc_", capi.ORACLE_EXTRAS)
    for name in ("orc_wavefront_load_flags", "orc_mat_disney", "orc_disney_params_default"):
        assert name not in api.missing, name
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint32)

    def bind(name, argtypes):
        fn = getattr(lib, "orcx_" + name)
        fn.restype, fn.argtypes = C.c_int32, argtypes
        setattr(api, "x_" + name, fn)
    bind("world_scatter", [C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, dp, dp, up,
                           C.c_uint64, C.c_void_p])
    bind("camera_rays", [C.c_void_p, C.POINTER(capi.RtCamera), C.c_uint64, dp, C.c_uint64])
    bind("disney_selftest", [C.c_int32, C.POINTER(capi.RtDisneyParams), dp, dp, dp, C.c_uint64])
    bind("world_radiance", [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, dp,
                            C.c_uint64, dp])
    bind("render_partials_loop", [C.c_void_p, C.c_int32, C.POINTER(capi.RtCamera), C.c_uint64, dp, C.c_uint64])
    return api


_TMP = []  # the temporary directories of this process (the driver, the written OBJ / MTL files): removed at its exit


def _tmpdir(prefix):
    tmp = tempfile.TemporaryDirectory(prefix=prefix)
    _TMP.append(tmp)
    return tmp.name


# ================================================================ A. Disney
R_FLOOR = math.sqrt(0.001)  # roughness^2 here is the 0.001 floor of calculate_anisotropic_params
IOR_THIN0 = 0.35 / 0.65     # thin_transmission_roughness' factor 0.65 ior - 0.35 is 0 (to an ulp) here

EDGE_SETS = {
    # roughness
    "rough_0": dict(roughness=0.0),
    "rough_1e-3": dict(roughness=1e-3),
    "rough_floor_lo": dict(roughness=nxt(R_FLOOR, False)),
    "rough_floor": dict(roughness=R_FLOOR),
    "rough_floor_hi": dict(roughness=nxt(R_FLOOR)),
    "rough_1": dict(roughness=1.0),
    "rough_2": dict(roughness=2.0),
    # anisotropic: aspect = sqrt(1 - 0.9 aniso) is 0 at 10/9 and NaN beyond
    "aniso_1": dict(anisotropic=1.0),
    "aniso_-1": dict(anisotropic=-1.0),
    "aniso_2": dict(anisotropic=2.0),
    "aniso_10/9_rough_0": dict(anisotropic=10.0 / 9.0, roughness=0.0),
    # the transmission lobe
    "trans_ior_1": dict(spec_trans=1.0, ior=1.0),
    "trans_ior_1+": dict(spec_trans=1.0, ior=nxt(1.0)),
    "trans_ior_0.5": dict(spec_trans=1.0, ior=0.5),
    "trans_ior_1e3": dict(spec_trans=1.0, ior=1e3),
    # thin (with a transmission weight, so that thin_transmission_roughness runs)
    "thin_ior_1": dict(thin=True, spec_trans=0.5, ior=1.0),
    "thin_ior_35/65": dict(thin=True, spec_trans=0.5, ior=IOR_THIN0),
    # clearcoat gloss: gtr1's a = lerp(0.1, 0.001, gloss)
    "coat_gloss_0": dict(clearcoat=1.0, clearcoat_gloss=0.0),
    "coat_gloss_1": dict(clearcoat=1.0, clearcoat_gloss=1.0),
    "coat_gloss_1.5": dict(clearcoat=1.0, clearcoat_gloss=1.5),
    "coat_gloss_-10": dict(clearcoat=1.0, clearcoat_gloss=-10.0),
    # clearcoat
    "coat_2": dict(clearcoat=2.0),
    "coat_-1": dict(clearcoat=-1.0),
    "coat_denormal": dict(clearcoat=5e-324),
    # the corners of (metallic, spec_trans)
    "corner_00": dict(metallic=0.0, spec_trans=0.0),
    "corner_01": dict(metallic=0.0, spec_trans=1.0),
    "corner_10": dict(metallic=1.0, spec_trans=0.0),
    "corner_11": dict(metallic=1.0, spec_trans=1.0),
    # a zero weight sum: norm = 1 / 0
    "metallic_2": dict(metallic=2.0),
    "trans_2": dict(spec_trans=2.0),
    # thin diffuse
    "thin_flat_0": dict(thin=True, flatness=0.0, diff_trans=0.0),
    "thin_flat_1": dict(thin=True, flatness=1.0, diff_trans=1.0),
    # sheen
    "sheen_-1": dict(sheen=-1.0),
    "sheen_tints_1": dict(sheen=1.0, sheen_tint=1.0, specular_tint=1.0),
    # finite parameters whose weights overflow to inf - inf: every lobe probability is NaN and generate()
    # reaches the reference's `panic!("The conditions should be exhausted!")`
    "weights_nan": dict(metallic=-1e200, spec_trans=1e200),
}
EDGE_NAMES = list(EDGE_SETS)
EDGE_COLORS = {"grey": (0.8, 0.8, 0.8), "black": (0.0, 0.0, 0.0), "gamut": (-0.5, 2.0, 0.3)}


def aniso_params(roughness, anisotropic):
    """calculate_anisotropic_params (disney.rs) in IEEE doubles, f64::max
    written out (NaN loses): (ax, ay, route) with route = 'floor' / 'nan' /
    None for how ax came to be 0.001 (or did not)."""
    with np.errstate(all="ignore"):
        aspect = np.sqrt(F(1.0) - F(0.9) * F(anisotropic))
        r2 = F(roughness) * F(roughness)
        qa, qb = r2 / aspect, r2 * aspect
    fmax = lambda a, b: a if np.isnan(b) else (b if np.isnan(a) else max(a, b))
    ax, ay = fmax(F(0.001), qa), fmax(F(0.001), qb)
    route = None
    if ax == 0.001:
        route = "nan" if np.isnan(qa) else "floor"
    return float(ax), float(ay), route


def gtr1_a(p):
    """gtr1's `a` for a parameter dict: lerp(0.1, 0.001, clearcoat_gloss) = a (1 - t) + b t."""
    t = F(p.get("clearcoat_gloss", 0.0))
    return float(F(0.1) * (F(1.0) - t) + F(0.001) * t)


@functools.lru_cache(maxsize=None)
def edge_gen_cases(name):
    return dq.gen_cases_for(EDGE_SETS[name], 1777 + EDGE_NAMES.index(name))


@functools.lru_cache(maxsize=None)
def oracle_selftest(fn, name, color):
    """orcx_disney_selftest of an edge set and colour name, computed once."""
    cases = dq.eval_cases() if fn == 0 else edge_gen_cases(name)
    out = dq.selftest(driver(), fn, EDGE_SETS[name], cases, oracle=True, color=EDGE_COLORS[color])
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------- the edge worlds
# The oracle's renderer, like the reference, ends at the first panic of a frame, so a frame can only be compared
# where no sample panics.  PANIC_MEMBERS panic in ray_color (trans_2: a NaN radiance, camera.rs:323;
# weights_nan: the exhausted conditions; thin with a negative base colour: `The answer of sqrt is NaN!`): they
# stand in world 3, which is compared record by record (rt_world_scatter, rt_world_radiance), not as a frame.
# Every other (set, colour) stands in one of worlds 0..2, sphere i of world k in colour (i + k) mod 3.
PANIC_SETS = ("trans_2", "weights_nan")
PANIC_MEMBERS = [("trans_2", "grey"), ("trans_2", "black"), ("weights_nan", "grey"), ("weights_nan", "gamut"),
                 ("thin_ior_1", "gamut"), ("thin_ior_35/65", "gamut")]
N_WORLDS = 4
RENDER_WORLDS = (0, 1, 2)
PANIC_WORLD = 3


def world_members(k):
    """[(edge set, colour name)] of world k."""
    if k == PANIC_WORLD:
        return list(PANIC_MEMBERS)
    names = [n for n in EDGE_NAMES if n not in PANIC_SETS][k::3]
    cols = list(EDGE_COLORS)
    out = []
    for i, n in enumerate(names):
        c = cols[(i + k) % 3]
        out.append((n, "grey" if (n, c) in PANIC_MEMBERS else c))
    return out


def edge_world(s, k):
    """Sky gradient, a Lambertian ground sphere and a BVH of unit spheres, one
    per member of world k, in two rows."""
    rt = pkg_module("raytracer")
    objs = s.Hittables()
    members = world_members(k)
    per_row = (len(members) + 1) // 2
    for i, (name, color) in enumerate(members):
        row, col = divmod(i, per_row)
        m = s.Disney(s.SolidColor(EDGE_COLORS[color]), **EDGE_SETS[name])
        objs.add(s.Sphere((-2.2 * (per_row - 1) / 2 + 2.2 * col, 1.0 + 2.1 * row, 0.3 * (i % 3) - 2.0 * row), 1.0, m))
    w = s.Hittables()
    w.add(s.Sphere((0.0, -1000.0, 0.0), 1000.0, s.Lambertian(s.SolidColor((0.5, 0.5, 0.5)))))
    w.add(s.BVH(objs))
    cam = dq._camera(rt, (0.0, 3.5, 17.0), (0.0, 1.8, 0.0), 30.0, s.SkyGradient())
    return w, None, cam


@functools.lru_cache(maxsize=None)
def edge_reference(k, seed=1):
    """The driver's render of edge world k: (linear, srgb, partials, panics,
    loop-order partials: orcx_render_partials_loop's, tests/cpp/edge_oracle.cpp)."""
    rt = pkg_module("raytracer")
    s = rt.Scene(driver())
    world, lights, cam = edge_world(s, k)
    lin, srgb, st = cam.render(world, lights, seed=seed)
    part, _ = cam.render_partials(world, lights, seed=seed)
    loop = np.zeros_like(part)
    c = cam.to_c()
    drv = driver()
    drv.check(drv.x_render_partials_loop(s.s, world.h, C.byref(c), int(seed), loop.ctypes.data_as(C.POINTER(C.c_double)),
                                         loop.size))
    for a in (lin, srgb, part, loop):
        a.setflags(write=False)
    return lin, srgb, part, int(st.panics), loop


@functools.lru_cache(maxsize=None)
def edge_scatter_reference(k):
    """(rays, eval_dirs, records) of orcx_world_scatter on the primary rays of edge world k's frame."""
    import radiance_query as rq
    rt = pkg_module("raytracer")
    drv = driver()
    s = rt.Scene(drv)
    world, _, cam = edge_world(s, k)
    rays = rq.camera_rays(drv, s, cam, seed=1)
    ev = np.random.default_rng(rq.RAY_SEED + k).standard_normal((len(rays), 3))
    ev /= np.linalg.norm(ev, axis=1)[:, None]
    want = sq.oracle_scatter(drv, s, world, rays, eval_dirs=ev, background=cam.background, vertex=1, sample=0)
    for a in (rays, ev, want):
        a.setflags(write=False)
    return rays, ev, want


@functools.lru_cache(maxsize=None)
def edge_radiance_reference(k, samples=4):
    """orcx_world_radiance (depth 8, `samples` a ray) on the same primary rays: (rgb, rays, panics)."""
    import radiance_query as rq
    rt = pkg_module("raytracer")
    drv = driver()
    s = rt.Scene(drv)
    world, _, cam = edge_world(s, k)
    rays = edge_scatter_reference(k)[0]
    out = rq.oracle_radiance(drv, s, world, None, rays, max_depth=dq.DEPTH, samples=samples, seed=rq.SEED,
                             background=cam.background)
    for a in out:
        a.setflags(write=False)
    return out


# ---------------------------------------------------------------- the MTL twin
# MTL keys that carry an edge set: Pr roughness, aniso, Ps sheen, Pm metallic, Pc clearcoat, Pcr clearcoat_gloss,
# Ni ior, Tf -> spec_trans = its mean.  Sets that use another field (thin, flatness, tints) have no MTL spelling.
MTL_KEY = {"roughness": "Pr", "anisotropic": "aniso", "sheen": "Ps", "metallic": "Pm", "clearcoat": "Pc",
           "clearcoat_gloss": "Pcr", "ior": "Ni"}


def mtl_sets():
    return [n for n in EDGE_NAMES if all(k in MTL_KEY or k == "spec_trans" for k in EDGE_SETS[n])]


def mtl_text_and_params(name):
    """(the MTL key lines {key: text}, the rt_mat_disney parameters they must
    load as) of an edge set.  Numbers are written with repr: the shortest
    text that reads back as the same double."""
    keys, params = {}, {}
    for k, v in EDGE_SETS[name].items():
        if k == "spec_trans":
            keys["Tf"] = "%r %r %r" % (v, v, v)
            params[k] = (0.0 + v + v + v) / 3.0  # obj.rs:266: the sum from 0 in order, over 3
        else:
            keys[MTL_KEY[k]] = repr(float(v))
            params[k] = float(v)
    return keys, params


def mtl_world_loaded(s, name, kd):
    world = s.Hittables()
    keys, _ = mtl_text_and_params(name)
    path = oq.write_tri(_tmpdir("edge_mtl_"), keys, kd, None)
    world.add(s.Wavefont(path, True, disney=True))  # RT_OBJ_VANILLA | RT_OBJ_DISNEY
    return world


def mtl_world_twin(s, name, kd):
    """The triangle built by hand.  With the vanilla flag the reference maps
    Pm == 1 to Metal(Kd, Pr) and a Tf mean == 1 to Dielectric(Kd, Ni)
    (obj.rs:271-278) before it considers Disney: the twin does the same."""
    _, params = mtl_text_and_params(name)
    if params.get("metallic") == 1.0:
        mat = s.Metal(kd, params.get("roughness", 0.5))
    elif params.get("spec_trans") == 1.0:
        mat = s.Dielectric(s.SolidColor(kd), params.get("ior", 1.45))
    else:
        mat = s.Disney(s.SolidColor(kd), **params)
    tris = s.Hittables()
    tris.add(s.Triangle(oq.TRI_A, oq.TRI_U, oq.TRI_V, mat))
    world = s.Hittables()
    world.add(s.BVH(tris))
    return world


# ================================================================ B. texture addressing
# ---- Rust's float -> integer casts (saturating, NaN -> 0), on int64 / uint64 arrays
def as_i32(x):
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), -2.0 ** 31, 2.0 ** 31 - 1.0))
    return t.astype(np.int64)


def as_u32(x):
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), 0.0, 2.0 ** 32 - 1.0))
    return t.astype(np.int64)


def as_i64(x):
    x = np.asarray(x, dtype=F)
    with np.errstate(invalid="ignore"):
        mid = np.where(np.isnan(x) | (np.abs(x) >= 2.0 ** 63), 0.0, np.trunc(x)).astype(np.int64)
    return np.where(x >= 2.0 ** 63, np.iinfo(np.int64).max, np.where(x <= -2.0 ** 63, np.iinfo(np.int64).min, mid))


def wrap_i32(x):
    """An exact integer sum brought back to i32 as a release build's wrapping add leaves it."""
    return (np.asarray(x, dtype=np.int64) + 2 ** 31) % 2 ** 32 - 2 ** 31


def checker_cells(scale, p):
    """texture.rs:61-63: the three `as i32` cells of points p (n, 3) under CheckerTexture::new(scale, ..)."""
    inv_scale = F(1.0) / F(scale)
    with np.errstate(all="ignore"):
        return as_i32(np.floor(inv_scale * np.asarray(p, dtype=F)))


def checker_is_even(scale, p):
    """texture.rs:65: (x_int + y_int + z_int) % 2 == 0, the sum wrapping; Rust's % keeps the dividend's sign."""
    c = checker_cells(scale, p)
    return wrap_i32(c[:, 0] + c[:, 1] + c[:, 2]) % 2 == 0


def image_texels(w, h):
    """h x w x 4 float32, every texel its own colour and alpha (all exact in
    f32): texel k = y w + x has blue (k + 1) / 32 and alpha (k + 1) / 64."""
    k = np.arange(w * h).reshape(h, w)
    img = np.empty((h, w, 4), dtype=np.float32)
    img[..., 0] = (1 + k % w) / 8.0
    img[..., 1] = (1 + k // w) / 8.0
    img[..., 2] = (k + 1) / 32.0
    img[..., 3] = (k + 1) / 64.0
    return img


def texel_id(blue):
    """The texel a nearest lookup returned, from image_texels' blue channel."""
    return np.rint(np.asarray(blue, dtype=F) * 32.0).astype(np.int64) - 1


def image_lookup(img, linear, u, v):
    """ImageTexture::get_pixel (texture.rs:111-158) on an (h, w, 4) float32
    image: (rgba (n, 4) float32, the intermediates the reach checks read)."""
    h, w = img.shape[:2]
    u, v = np.asarray(u, dtype=F), np.asarray(v, dtype=F)
    with np.errstate(invalid="ignore"):
        uu = u - np.floor(u)                 # abs_fract
        vv = F(1.0) - (v - np.floor(v))

        def pix(x, y):                        # image.rs:63-82: u32 clamp
            return img[np.minimum(y, h - 1), np.minimum(x, w - 1)]
        if not linear:
            i, j = as_u32(uu * F(w)), as_u32(vv * F(h))
            return pix(i, j), dict(uu=uu, vv=vv, i=i, j=j)
        x, y = uu * F(w) - F(0.5), vv * F(h) - F(0.5)
        fx, fy = np.floor(x), np.floor(y)
        x0 = as_u32(np.where(np.isnan(fx), 0.0, np.maximum(fx, 0.0)))  # f64::max: NaN loses
        y0 = as_u32(np.where(np.isnan(fy), 0.0, np.maximum(fy, 0.0)))
        x1 = np.minimum((x0 + 1) % 2 ** 32, w - 1)
        y1 = np.minimum((y0 + 1) % 2 ** 32, h - 1)
        dx = (x - x0.astype(F)).astype(np.float32)[:, None]
        dy = (y - y0.astype(F)).astype(np.float32)[:, None]
        one = np.float32(1.0)
        p00, p10, p01, p11 = pix(x0, y0), pix(x1, y0), pix(x0, y1), pix(x1, y1)
        v0 = p00 * (one - dx) + p10 * dx
        v1 = p01 * (one - dx) + p11 * dx
        out = v0 * (one - dy) + v1 * dy
    assert out.dtype == np.float32
    return out, dict(uu=uu, vv=vv, x=x, y=y, x0=x0, x1=x1, y0=y0, y1=y1, dx=dx[:, 0], dy=dy[:, 0])


# ---- texture descriptions: ("solid", rgb) / ("image", (w, h), linear) / ("checker", scale, even, odd) /
#      ("noise", scale, seed)
def build_tex(s, d):
    if d[0] == "solid":
        return s.SolidColor(d[1])
    if d[0] == "image":
        return s.ImageTexture(image_texels(*d[1]), linear_interp=d[2])
    if d[0] == "checker":
        return s.CheckerTexture(d[1], build_tex(s, d[2]), build_tex(s, d[3]))
    if d[0] == "noise":
        return s.NoiseTexture(d[1], d[2])
    raise ValueError(d[0])


def has_noise(d):
    return d[0] == "noise" or (d[0] == "checker" and (has_noise(d[2]) or has_noise(d[3])))


def model_value(d, u, v, p):
    """Texture::value of a description at (u, v, p): (n, 3) float64.  NoiseTexture has no model."""
    n = len(u)
    if d[0] == "solid":
        return np.tile(np.asarray(d[1], dtype=F), (n, 1))
    if d[0] == "image":
        return image_lookup(image_texels(*d[1]), d[2], u, v)[0][:, :3].astype(F)
    if d[0] == "checker":
        even = checker_is_even(d[1], p)
        return np.where(even[:, None], model_value(d[2], u, v, p), model_value(d[3], u, v, p))
    raise ValueError(d[0])


def model_alpha(d, u, v):
    """ImageTexture::alpha (texture.rs:102-109)."""
    return image_lookup(image_texels(*d[1]), d[2], u, v)[0][:, 3].astype(F)


# ---- probe groups
IMAGE_SIZES = ((1, 1), (1, 5), (5, 1), (4, 3))
BIG = (2.0 ** 31, 2.0 ** 40, 2.0 ** 52, 2.0 ** 62, 2.0 ** 63)
NOISE_BIG = BIG[:4]  # Perlin at or beyond 2^63 is out of scope (Rust wraps i + 1 there)


def _near(x):
    return [nxt(x, False), x, nxt(x)]


def coord_edges(n):
    """The texture coordinates of an axis with n texels, within the unit quad."""
    c = [0.0, 5e-324, 1.0 - 2.0 ** -53, 1.0] + _near(1.0 / (2 * n))
    for k in range(n + 1):
        c += _near(k / n)
    return sorted({x for x in c if 0.0 <= x <= 1.0})


def _rays(points, z, t_max=np.inf):
    """Rays (x, y, z + 1) -> -z onto the plane z: they arrive with t = 1 and p = (x, y, z) exactly."""
    pts = np.asarray(points, dtype=F).reshape(-1, 2)
    r = np.zeros((len(pts), 8))
    r[:, 0:2] = pts
    r[:, 2] = z + 1.0
    r[:, 5] = -1.0
    r[:, 6] = 0.5
    r[:, 7] = t_max
    return r


def _grid(xs, ys):
    return [(x, y) for x in xs for y in ys]


def quad_groups():
    """[dict(name, tex, quad = (Q, u, v), rays)]: one emitting quad a group, in the plane z = -3 (k + 1)."""
    groups = []

    def add(name, tex, lo, size, points):
        z = -3.0 * (len(groups) + 1)
        groups.append(dict(name=name, kind="quad", tex=tex, z=z, quad=((lo, lo, z), (size, 0.0, 0.0), (0.0, size, 0.0)),
                           rays=_rays(points, z)))

    for w, h in IMAGE_SIZES:
        for linear in (False, True):
            add(f"image_{w}x{h}_{'bilinear' if linear else 'nearest'}", ("image", (w, h), linear), 0.0, 1.0,
                _grid(coord_edges(w), coord_edges(h)))
    # the checker's `as i32`, by the scale: floor(inv_scale * p) = T exactly, p within (-2, 2)
    img_a, img_b = ("image", (4, 3), False), ("image", (5, 1), True)
    a, b = ("solid", (1.0, 0.25, 0.0)), ("solid", (0.0, 0.5, 1.0))
    t31 = [s * t for t in (2.0 ** 31 - 1, 2.0 ** 31, 2.0 ** 31 + 1) for s in (1.0, -1.0)]
    others = [0.25, -0.75, 2.0 ** -31, -2.0 ** -31]
    add("checker_2^-31", ("checker", 2.0 ** -31, a, b), -2.0, 4.0,
        _grid([t / 2.0 ** 31 for t in t31] + others, others) + _grid(others, [t / 2.0 ** 31 for t in t31]))
    t62 = [s * t for t in (2.0 ** 40, 2.0 ** 52, 2.0 ** 62, 2.0 ** 63) for s in (1.0, -1.0)]
    small = [2.0 ** -62, -2.0 ** -62, 2.0 ** -61, -2.0 ** -61]
    add("checker_2^-62", ("checker", 2.0 ** -62, a, b), -2.0, 4.0,
        _grid([t / 2.0 ** 62 for t in t62] + small, small) + _grid(small, [t / 2.0 ** 62 for t in t62]))
    add("checker_1e-300", ("checker", 1e-300, a, b), -2.0, 4.0, _grid([1.0, -1.0, 1e-300, -1e-300], [1.0, -1.0, 1e-300]))
    # negative odd and even cells next to 0
    cells = [-2.5, -2.0, -1.5, -1.0, -0.5, -1e-300, -0.0, 0.0, 5e-324, 0.5, 1.0, 1.5]
    add("checker_cells", ("checker", 1.0, a, b), -4.0, 8.0, _grid(cells, cells))
    # a checker of checkers of images: the texture loop, with (u, v) carried through
    nested = ("checker", 0.5, ("checker", 0.25, img_a, img_b), ("checker", 1.0 / 3.0, ("image", (1, 5), True), a))
    add("checker_nested", nested, 0.0, 1.0, _grid(coord_edges(4), coord_edges(3)))
    # the same casts with p itself large: a quad of side 4 M about the origin
    for m in BIG:
        xs = [s * t for t in ((m - 1, m, m + 1) if m == 2.0 ** 31 else (m,)) for s in (1.0, -1.0)]
        ys = [0.5, -1.5, m, -m]
        add(f"checker_at_{m:g}", ("checker", 1.0, a, b), -2.0 * m, 4.0 * m, _grid(xs, ys) + _grid(ys, xs))
        if m in NOISE_BIG:
            add(f"noise_at_{m:g}", ("noise", 4.0, 3), -2.0 * m, 4.0 * m, _grid(xs, ys) + _grid(ys, xs))
    g = np.random.default_rng(20251022)
    add("noise_near_0", ("noise", 4.0, 3), -4.0, 8.0, g.uniform(-4.0, 4.0, (96, 2)))
    return groups


# spheres stand at (100, 100 i, 0): seam rays travel along x, pole rays along y, none crosses a quad's plane
SPHERE_RADII = (1.0, 0.3, 1.0 / 3.0, 1e-3, 0.7, 2.5, 0.1, 3.0)


def sphere_groups():
    groups = []
    for i, r in enumerate(SPHERE_RADII):
        w, h = IMAGE_SIZES[i % 4]
        c = np.array([100.0, 100.0 * i, 0.0])
        rays = []
        # the poles: straight down / up the axis, and a few ulp off it, from several heights
        for k in range(12):
            for sgn in (1.0, -1.0):
                for dxz in ((0.0, 0.0), (r * 2.0 ** -30, 0.0), (0.0, -r * 2.0 ** -30)):
                    o = c + np.array([dxz[0], sgn * r * (2.0 + 0.37 * k), dxz[1]])
                    rays.append([*o, 0.0, -sgn * (1.0 + 0.13 * k), 0.0, 0.5, np.inf])
        # the seam half-plane x < 0, z = +-0: along +x at several heights, z and d.z = +-0 and a few ulp either side
        for y in (0.0, 0.3 * r, -0.6 * r, 0.9 * r):
            for z in (0.0, -0.0, 5e-324, -5e-324, r * 2.0 ** -52, -r * 2.0 ** -52, r * 2.0 ** -40, -r * 2.0 ** -40):
                for dz in (0.0, -0.0):
                    rays.append([c[0] - 5.0, c[1] + y, z, 1.0, 0.0, dz, 0.5, np.inf])
        groups.append(dict(name=f"sphere_r{r:g}", kind="sphere", tex=("image", (w, h), (i // 4 + i) % 2 == 1),
                           center=tuple(c), radius=r, rays=np.array(rays, dtype=F)))
    return groups


ENV_ORIGIN = (0.0, 1.0e5, 7.0)


def env_rays():
    """Rays that miss (an empty interval: t_max below 1e-8): the six axis
    directions, the environment's seam and poles, and directions of length
    1e-150 and 1e150."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    off_seam = (0.0, -0.0, 5e-324, -5e-324, 2.0 ** -52, -2.0 ** -52, 2.0 ** -30, -2.0 ** -30)
    dirs += [(-1.0, y, z) for y in (0.0, 0.5, -2.0) for z in off_seam]
    dirs += [(x, y, z) for y in (1.0, -1.0) for x in (0.0, -0.0, 2.0 ** -30, 2.0 ** -20) for z in (0.0, -0.0)]
    g = np.random.default_rng(20251023)
    rnd = g.standard_normal((64, 3))
    out = []
    for d in dirs:
        for scale in (1.0, 1e-150, 1e150):
            out.append([*ENV_ORIGIN, *(np.array(d, dtype=F) * scale), 0.5, 1e-9])
    for d in rnd:
        for scale in (1.0, 1e-150, 1e150):
            out.append([*ENV_ORIGIN, *(d * scale), 0.5, 1e-9])
    return np.array(out, dtype=F)


ENV_TEX = ("image", (4, 3), True)
AXIS_ENV = 6 * 3  # env_rays()' first rows: the axis directions at the three lengths


@functools.lru_cache(maxsize=None)
def probe_groups():
    groups = quad_groups() + sphere_groups()
    start = 0
    for g in groups:
        g["rays"].setflags(write=False)
        g["slice"] = slice(start, start + len(g["rays"]))
        start += len(g["rays"])
    return groups


@functools.lru_cache(maxsize=None)
def probe_rays():
    """(the groups' rays then the environment's, the index where the environment's begin)."""
    r = np.concatenate([g["rays"] for g in probe_groups()] + [env_rays()])
    r.setflags(write=False)
    return r, len(r) - len(env_rays())


TIERS = (2, 3, 4, 5)


def probe_world(s, tier):
    """Every probe group as a DiffuseLight(texture) object in one flat list,
    plus what makes the flattening take kernel tier `tier`: nothing (3: the
    flat full tier), a BVH node (2), a Mix::from_image object (4), a Disney
    sphere (5) -- none of them in a probe ray's way.  Returns (world, background)."""
    w = s.Hittables()
    for g in probe_groups():
        m = s.DiffuseLight(build_tex(s, g["tex"]))
        w.add(s.Quad(*g["quad"], m) if g["kind"] == "quad" else s.Sphere(g["center"], g["radius"], m))
    grey = s.SolidColor((0.5, 0.5, 0.5))
    if tier == 2:
        b = s.Hittables()
        b.add(s.Sphere((0.0, 50.0, 0.0), 1.0, s.Lambertian(grey)))
        w.add(s.BVH(b))
    elif tier == 4:
        veil = s.Mix_from_image(s.Transparent(), s.Lambertian(grey), build_tex(s, ("image", (4, 3), False)))
        w.add(s.Sphere((0.0, 50.0, 0.0), 1.0, veil))
    elif tier == 5:
        w.add(s.Sphere((0.0, 50.0, 0.0), 1.0, s.Disney(grey)))
    elif tier != 3:
        raise ValueError(tier)
    return w, build_tex(s, ENV_TEX)


@functools.lru_cache(maxsize=None)
def probe_reference():
    """orcx_world_scatter and orcx_world_radiance (depth 1) of every probe ray on the oracle: (records, rgb)."""
    import radiance_query as rq
    rt = pkg_module("raytracer")
    drv = driver()
    s = rt.Scene(drv)
    world, bg = probe_world(s, 3)
    rays, _ = probe_rays()
    want = sq.oracle_scatter(drv, s, world, rays, background=bg, seed=rq.SEED)
    rgb, _, panics = rq.oracle_radiance(drv, s, world, None, rays, max_depth=1, samples=1, seed=rq.SEED, background=bg)
    for a in (want, rgb, panics):
        a.setflags(write=False)
    return want, rgb, panics


def env_uv(d):
    """Environment::value's own (u, v, p) (environment.rs: phi = pi - atan2(-z, x)) for directions d (n, 3),
    in numpy's libm: exact at the axis directions, where every argument is a signed zero or +-1."""
    d = np.asarray(d, dtype=F)
    p = d / np.sqrt((d * d).sum(axis=1))[:, None]
    theta = np.arccos(-p[:, 1])
    phi = np.pi - np.arctan2(-p[:, 2], p[:, 0])
    return phi / (2.0 * np.pi), theta / np.pi, p


# ---------------------------------------------------------------- OBJ triangles with constant texture coordinates
# All three vt of a triangle are one constant (cu, cv): tex_u = tex_v = 0 and remap_record hands the texture
# exactly (cu, cv) wherever the ray lands.  The images are 4 x 2 PNGs of bytes 0 / 255 (exactly 0.0 / 1.0 after the
# sRGB decode): ke.png's texel k = y w + x has (r, g, b) = the three bits of k, d.png's alpha is 255 where k % 3 == 0.
OBJ_W, OBJ_H = 4, 2
OBJ_C = (-1e-20, -2.0, -1.0, 0.0, 1.0, 2.0, 2.0 ** 52 + 0.5, -2.0 ** 53, 1e300, -1e300)
OBJ_FIXED_U, OBJ_FIXED_V = 0.6, 0.3   # column int(0.6 * 4) = 2, row int((1 - 0.3) * 2) = 1


def obj_texels():
    """(ke (h, w, 4), d (h, w, 4)) float32 as the decoders give them."""
    k = np.arange(OBJ_W * OBJ_H).reshape(OBJ_H, OBJ_W)
    ke = np.stack([(k >> 0) & 1, (k >> 1) & 1, (k >> 2) & 1, np.ones_like(k)], axis=-1).astype(np.float32)
    d = np.stack([np.ones_like(k), np.zeros_like(k), np.ones_like(k), (k % 3 == 0).astype(int)], axis=-1).astype(np.float32)
    return ke, d


def obj_cases():
    """[(cu, cv, with_map_d)]: triangle t of the file."""
    out = []
    for veil in (False, True):
        out += [(c, OBJ_FIXED_V, veil) for c in OBJ_C] + [(OBJ_FIXED_U, c, veil) for c in OBJ_C]
    return out


def obj_expected_texel(cu, cv):
    """The texel (column, row) a nearest lookup at (cu, cv) reads, in closed
    form: abs_fract(-1e-20) is 1.0 (column w, clamped to w - 1; row 0), every
    other constant here has fraction 0 (column 0; 1 - 0 = 1 -> row h, clamped
    to h - 1); 2^52 + 0.5 is 2^52 as a double."""
    col = 2 if cu == OBJ_FIXED_U else (OBJ_W - 1 if cu == -1e-20 else 0)
    row = 1 if cv == OBJ_FIXED_V else (0 if cv == -1e-20 else OBJ_H - 1)
    return col, row


@functools.lru_cache(maxsize=None)
def obj_dir():
    from PIL import Image
    d = _tmpdir("edge_obj_")
    ke, al = obj_texels()
    Image.fromarray((ke[..., :3] * 255).astype(np.uint8), "RGB").save(os.path.join(d, "ke.png"))
    Image.fromarray((al * 255).astype(np.uint8), "RGBA").save(os.path.join(d, "d.png"))
    obj, mtl = ["mtllib e.mtl", "vn 0 0 1"], []
    for t, (cu, cv, veil) in enumerate(obj_cases()):
        x = 3.0 * t
        obj += ["v %r 0 0" % x, "v %r 0 0" % (x + 2.0), "v %r 2 0" % x, "vt %r %r" % (float(cu), float(cv)), "o t%d" % t,
                "usemtl m%d" % t, "f %d/%d/1 %d/%d/1 %d/%d/1" % (3 * t + 1, t + 1, 3 * t + 2, t + 1, 3 * t + 3, t + 1)]
        mtl += ["newmtl m%d" % t, "Kd 0.5 0.5 0.5", "map_Ke ke.png"] + (["map_d d.png"] if veil else [])
    with open(os.path.join(d, "e.obj"), "w") as f:
        f.write("\n".join(obj) + "\n")
    with open(os.path.join(d, "e.mtl"), "w") as f:
        f.write("\n".join(mtl) + "\n")
    return d


def obj_world(s):
    """The file loaded with RT_OBJ_VANILLA | RT_OBJ_DISNEY under a sky gradient; a camera that sees every triangle."""
    rt = pkg_module("raytracer")
    world = s.Hittables()
    world.add(s.Wavefont(os.path.join(obj_dir(), "e.obj"), True, disney=True))
    n = len(obj_cases())
    cam = rt.Camera()
    cam.aspect_ratio, cam.image_width, cam.samples_per_pixel, cam.max_depth = 16 / 9, 16, 4, 8
    cam.vertical_fov_in_degrees = 40.0
    mid = 3.0 * (n - 1) / 2 + 1.0
    cam.look_from, cam.look_at, cam.vec_up = (mid, 1.0, 95.0), (mid, 1.0, 0.0), (0.0, 1.0, 0.0)
    cam.background = s.SkyGradient()
    return world, None, cam


@functools.lru_cache(maxsize=None)
def obj_rays():
    """Six rays a triangle, (x, y, 1) -> -z, well inside it: (rays, the triangle of each)."""
    g = np.random.default_rng(20251024)
    pts, tri = [], []
    for t in range(len(obj_cases())):
        for _ in range(6):
            a, b = g.uniform(0.1, 0.8, 2)
            if a + b > 0.9:
                a, b = 0.9 - b, 0.9 - a
            pts.append((3.0 * t + 2.0 * a, 2.0 * b))
            tri.append(t)
    r = _rays(pts, 0.0)
    r.setflags(write=False)
    return r, np.array(tri)


def obj_model(tri):
    """The emitted colour of a hit on each triangle of `tri`: DiffuseLight(ke)
    at (cu, cv), under Mix::from_image(Transparent, .., d) times d's alpha."""
    ke, al = obj_texels()
    cases = obj_cases()
    cu = np.array([cases[t][0] for t in tri], dtype=F)
    cv = np.array([cases[t][1] for t in tri], dtype=F)
    veil = np.array([cases[t][2] for t in tri])
    e, m = image_lookup(ke, False, cu, cv)
    a = image_lookup(al, False, cu, cv)[0][:, 3].astype(F)
    e = e[:, :3].astype(F)
    # Mix::emitted: mat1.emitted * (1 - r) + mat2.emitted * r, Transparent emitting nothing
    return np.where(veil[:, None], np.zeros_like(e) * (F(1.0) - a)[:, None] + e * a[:, None], e), m


@functools.lru_cache(maxsize=None)
def obj_reference():
    """(scatter records of obj_rays(), partials of the 16 x 9 x 4 spp frame, linear, panics) on the oracle."""
    import radiance_query as rq
    rt = pkg_module("raytracer")
    drv = driver()
    s = rt.Scene(drv)
    world, _, cam = obj_world(s)
    want = sq.oracle_scatter(drv, s, world, obj_rays()[0], background=cam.background, seed=rq.SEED)
    lin, _, st = cam.render(world, None, seed=1)
    part, _ = cam.render_partials(world, None, seed=1)
    for a in (want, lin, part):
        a.setflags(write=False)
    return want, part, lin, int(st.panics)


def differing_fields(got, want):
    """scatter_query.differing_fields with NaN equal to NaN: name -> indices of the records that differ."""
    bad = {}

    def note(name, same):
        d = ~np.asarray(same).reshape(len(got), -1).all(axis=1)
        if d.any():
            bad[name] = np.nonzero(d)[0]
    for k in sq.FLOAT_FIELDS:
        note(k, dq.same_bits(got[k], want[k]))
    for k in sq.HIT_FLOAT_FIELDS:
        note("hit." + k, dq.same_bits(got["hit"][k], want["hit"][k]))
    for k in ("flags", "draws"):
        note(k, got[k] == want[k])
    note("hit.flags", got["hit"]["flags"] == want["hit"]["flags"])
    return bad
