"""The Disney BSDF without a GPU: rtcr::pow_2m4 against libquadmath, the
rt_mat_disney ABI and its flattening (tier 5, F_DISNEY, wrappers), and sanity
checks of the test-side restatement (tests/cpp/disney_oracle.cpp) that guard
against a mis-transcribed branch.  Fidelity to disney.rs otherwise rests on
review of the cited lines: the reference cannot be run here.
"""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import disney_query as dq


# ---------------------------------------------------------------- pow_2m4
@pytest.fixture(scope="module")
def pow_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("pow_check")
    src = os.path.join(ROOT, "tests", "cpp", "pow_check.cpp")
    out = {}
    for name, flags in (("plain", ["-ffp-contract=off"]), ("fma", ["-ffp-contract=fast", "-mfma"])):
        exe = str(d / ("pow_check_" + name))
        subprocess.run(["g++", "-O2", "-std=c++17"] + flags + [src, "-lquadmath", "-o", exe], check=True, timeout=300)
        out[name] = exe
    return out


@pytest.mark.parametrize("build", ["plain", "fma"])
def test_pow_2m4_correctly_rounded(pow_check, build):
    """0.0625^y for 60 000 unit draws, y = 0, 1, k/4, the smallest and largest
    draws and the steps of the table, with and without host FMA contraction:
    zero misrounded against powq (the bar of tests/cpp/crmath_check.cpp)."""
    r = json.loads(subprocess.run([pow_check[build], "60000"], check=True, capture_output=True, text=True,
                                  timeout=300).stdout)
    print(f"pow_2m4 [{build}]: n {r['n']}, misrounded {r['cr_not_correctly_rounded']}, glibc pow misrounded "
          f"{r['glibc_not_correctly_rounded']} ({r['glibc_not_correctly_rounded'] / r['n']:.2e}), slow path "
          f"{r['slow_path']} ({r['slow_path'] / r['n']:.2e})")
    assert r["n_draws"] == 60000
    assert r["cr_not_correctly_rounded"] == 0, r
    assert r["exact_powers_bad"] == 0
    assert r["outside_domain_nan"] is True


# ---------------------------------------------------------------- ABI
DEFAULTS = dict(roughness=0.5, anisotropic=0.0, sheen=0.0, sheen_tint=0.0, clearcoat=0.0, clearcoat_gloss=0.0,
                specular_tint=0.0, metallic=0.0, ior=1.45, flatness=0.0, spec_trans=0.0, diff_trans=0.0, thin=0)


def test_defaults_are_the_reference(product, capi):
    """rt_disney_params_default = DisneyParameters::default (disney.rs:36-55); the restatement's too."""
    for api in (product, dq.driver()):
        p = capi.RtDisneyParams()
        api.disney_params_default(C.byref(p))
        assert p.struct_size == C.sizeof(capi.RtDisneyParams) == 104
        assert {k: getattr(p, k) for k in DEFAULTS} == DEFAULTS


def test_error_codes(product, capi, rt):
    s = rt.Scene(product)
    tex = s.SolidColor((0.8, 0.8, 0.8))
    p = s.disney_params()
    assert product.mat_disney(s.s, tex.h, C.byref(p)) >= 0
    assert product.mat_disney(s.s, tex.h, None) == -1
    assert product.mat_disney(None, tex.h, C.byref(p)) == -1
    assert product.mat_disney(s.s, 99, C.byref(p)) == -2
    assert product.mat_disney(s.s, -1, C.byref(p)) == -2
    short = s.disney_params()
    short.struct_size = C.sizeof(capi.RtDisneyParams) - 8
    assert product.mat_disney(s.s, tex.h, C.byref(short)) == -1
    for field in ("roughness", "ior", "diff_trans"):
        for bad in (math.nan, math.inf, -math.inf):
            q = s.disney_params(**{field: bad})
            assert product.mat_disney(s.s, tex.h, C.byref(q)) == -1, (field, bad)
    # ranges are not checked, as the reference checks none
    assert product.mat_disney(s.s, tex.h, C.byref(s.disney_params(roughness=-3.0, metallic=7.0))) >= 0
    with pytest.raises(TypeError):
        s.Disney(tex, glossiness=1.0)


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
    """A one-sphere Disney world is tier 5 with F_DISNEY; the same world with
    Lambertian reports what it reports without this material: tier 0, no bit."""
    f_disney = dq.feature_bit("F_DISNEY")
    s = rt.Scene(product)
    tex = s.SolidColor((0.8, 0.8, 0.8))
    d = _info(product, capi, s, _one_sphere(s, s.Disney(tex)))
    assert d.kernel_tier == 5 and d.features & f_disney
    lam = _info(product, capi, s, _one_sphere(s, s.Lambertian(tex)))
    assert lam.kernel_tier == 0 and not lam.features & f_disney
    assert d.features == lam.features | f_disney
    assert (d.primitives, d.bvh_nodes, d.stack_need) == (lam.primitives, lam.bvh_nodes, lam.stack_need)
    # an unused Disney material does not move the tier
    assert _info(product, capi, s, _one_sphere(s, s.Lambertian(tex))).kernel_tier == 0


def test_tier_for_keeps_every_other_combination(product):
    """tier_for returns 5 exactly when F_DISNEY is set, and what it returned before otherwise."""
    names = ("F_XFORM", "F_MEDIUM", "F_PLANAR", "F_MSPHERE", "F_LIGHTS", "F_TEXFULL", "F_MATFULL", "F_REMAP", "F_NORMALMAP",
             "F_GENERAL")
    bit = {n: dq.feature_bit(n) for n in names}
    f_disney = dq.feature_bit("F_DISNEY")
    assert f_disney not in bit.values()
    full = sum(bit[n] for n in ("F_XFORM", "F_MEDIUM", "F_MSPHERE", "F_LIGHTS", "F_TEXFULL", "F_MATFULL", "F_NORMALMAP"))
    fn = product.lib.rtk_tier_for
    fn.restype, fn.argtypes = C.c_int, [C.c_uint32]
    for f in range(1024):
        want = 4 if f & bit["F_GENERAL"] else 2 if f & full else 1 if f & (bit["F_PLANAR"] | bit["F_REMAP"]) else 0
        assert fn(f) == want, f
        assert fn(f | f_disney) == 5, f


def test_disney_under_wrappers(product, capi, rt):
    """Disney as a Mix / DiffuseLight inner material is accepted (tier 5, emission found through the wrapper);
    five wrapper levels are still refused."""
    s = rt.Scene(product)
    tex = s.SolidColor((0.8, 0.8, 0.8))
    dis = s.Disney(tex, clearcoat=1.0)
    for m in (s.Mix(s.Transparent(), dis, 0.5), s.DiffuseLight(tex, dis), s.Mix(dis, s.DiffuseLight(tex, dis), 0.25)):
        assert _info(product, capi, s, _one_sphere(s, m)).kernel_tier == 5
    m = dis
    for _ in range(4):
        m = s.DiffuseLight(tex, m)
    assert _info(product, capi, s, _one_sphere(s, m)).kernel_tier == 5
    m = s.DiffuseLight(tex, m)
    info = capi.RtWorldInfo()
    assert product.world_info_get(s.s, _one_sphere(s, m).h, -1, -1, 0, C.byref(info)) == -6


def test_selftest_args_without_a_device(product, rt):
    """rt_disney_selftest's argument checks come before any device work."""
    s = rt.Scene(product)
    p = s.disney_params()
    base = (C.c_double * 3)(0.8, 0.8, 0.8)
    buf = (C.c_double * 16)()
    assert product.disney_selftest(2, C.byref(p), base, buf, buf, 1) == -1
    assert product.disney_selftest(0, None, base, buf, buf, 1) == -1
    assert product.disney_selftest(0, C.byref(p), None, buf, buf, 1) == -1
    assert product.disney_selftest(0, C.byref(p), base, None, buf, 1) == -1
    assert product.disney_selftest(0, C.byref(p), base, None, None, 0) == 0
    nanbuf = (C.c_double * 1)(0.5)
    out = (C.c_double * 1)()
    assert product.math_selftest(11, 0, nanbuf, None, out, 1) == -1


# ---------------------------------------------------------------- the restatement
def _eval(name, v_out, v_in, front=1.0, **over):
    drv = dq.driver()
    a = np.array([[*v_out, *v_in, front]], dtype=np.float64)
    p = dq.params_struct(drv, **dict(dq.PARAM_SETS[name], **over))
    base = (C.c_double * 3)(*dq.COLORS[name])
    out = np.zeros((1, 6))
    dp = C.POINTER(C.c_double)
    drv.check(drv.x_disney_selftest(0, C.byref(p), base, a.ctypes.data_as(dp), out.ctypes.data_as(dp), 1))
    return out[0]


def test_restatement_default_mirror_direction():
    """Default parameters, v_out at 45 degrees: evaluate_disney at the mirror
    direction is finite and positive with a finite forward pdf."""
    c = math.sqrt(0.5)
    r = _eval("default", (c, c, 0.0), (-c, c, 0.0))
    assert r[5] == 0.0
    assert np.isfinite(r[:5]).all() and (r[:3] > 0.0).all() and r[3] > 0.0 and r[4] > 0.0


def test_restatement_metallic_has_no_diffuse_lobe():
    """metallic = 1: the diffuse (and transmission) lobe probabilities are 0 --
    every first draw in [0, 1) takes the specular sampler (three draws), and
    the running sums say so."""
    ps, ps_pc, ps_pd_pc = dq.lobe_sums(dict(metallic=1.0))
    assert ps == 1.0 and ps_pd_pc - ps_pc == 0.0
    drv = dq.driver()
    rows = np.array([[0.0, 1.0, 0.0, 0.3, 0.8, 0.2, 1.0, p, 0.37, 0.61, 0.5] for p in (0.0, 0.5, 0.999999)])
    out = dq.selftest(drv, 1, "metal", rows, oracle=True)
    assert (out[:, 5] == 0.0).all() and (out[:, 4] == 3.0).all()
    # and with diffuse weight the same draws past p_specular take the diffuse sampler (four draws)
    d = dq.selftest(drv, 1, "default", rows[2:], oracle=True)
    assert d[0, 4] == 4.0


def test_restatement_transmission_reaches_the_lower_hemisphere():
    """spec_trans = 1, metallic = 0: a direction in the lower hemisphere has non-zero reflectance."""
    c = math.sqrt(0.5)
    r = _eval("glass", (c, c, 0.0), (-0.3, -math.sqrt(1.0 - 0.09), 0.0))
    assert r[5] == 0.0 and (r[:3] > 0.0).all() and np.isfinite(r[3]) and r[3] > 0.0
    # a metal has nothing there
    z = _eval("metal", (c, c, 0.0), (-0.3, -math.sqrt(1.0 - 0.09), 0.0))
    assert z[5] == 0.0 and (z[:3] == 0.0).all()


def test_restatement_panics_and_quirks():
    """v_in = -v_out in the tangent plane panics (the half vector: with y = 0 the pair is no
    transmission, so the sum is normalised, and it is zero; off the plane v_in - v_out is not);
    a zero forward pdf is +inf, not a panic."""
    c = math.sqrt(0.5)
    assert _eval("default", (c, 0.0, c), (-c, 0.0, -c))[5] == 1.0
    assert _eval("default", (c, c, 0.0), (-c, -c, 0.0))[5] == 0.0
    # metallic: below the surface nothing is evaluated: forward pdf 0 -> +inf
    r = _eval("metal", (c, c, 0.0), (0.6, -0.8, 0.0))
    assert r[5] == 0.0 and (r[:3] == 0.0).all() and r[3] == math.inf


@pytest.mark.parametrize("name", list(dq.WORLDS))
def test_render_worlds_do_not_panic_on_the_restatement(name):
    """The GPU tests' worlds are chosen so that the restatement reports no panic."""
    lin, _, part, panics = dq.reference(name)
    assert panics == 0
    assert np.isfinite(lin).all() and lin.shape == (18, 32, 3) and lin.max() > 0.0
