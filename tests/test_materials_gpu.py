"""GPU parity for the material and texture code of the three full tiers
(rt_shade.h, rt_record.h, rt_texture.h, the flag resolution of the flatten)
on worlds made directly, not through the OBJ loader: Mix, Mix::from_image,
Transparent, Isotropic on a surface and DiffuseLight with a wrapped material
on spheres, moving spheres and quads, where a wrapped texture's (u, v) exists
only if MF_NEEDS_UV was lifted into the wrapper; wrapper trees of depth 2 to
4 (tier FULL_GL); and NoiseTextures past the first, whose tables are read
from global memory, on every full tier, as a checker child, a light's and a
medium's texture and the environment, and at negative lattice coordinates.

The worlds are tests/material_worlds.py's.  Each renders on the kernel and on
the TEST-ONLY oracle from the same scene script and seed; bars as
test_parity_gpu.check's defaults (RMSE < 1e-5, 0.999 of the pixels within
1e-5, at most 1e-3 of the (pixel, s_i) sums diverged), no panic on either
side, and the kernel tier asserted so that a scene cannot drift onto another
kernel.  The furnace and emission worlds are also held to closed-form answers
the oracle has no part in."""
import numpy as np
import pytest

import material_worlds as mw
from test_lights_textures_gpu import _tier
from test_parity_gpu import check, render_both

pytestmark = pytest.mark.gpu


def _parity(gpu, oracle, rt, capi, name):
    out, st = render_both(gpu, oracle, rt, lambda s: mw.build(rt, s, name))
    print(name, end=": ")
    check(out)
    assert st["gpu"].panics == st["oracle"].panics == 0
    s = rt.Scene(gpu)
    w, l, c = mw.build(rt, s, name)
    assert _tier(gpu, capi, s, w, l, c) == mw.expected(name)[0]
    return out


@pytest.mark.parametrize("name", list(mw.CASES))
def test_material_world(gpu, oracle, rt, capi, name):
    """<family>_<flat|bvh>_<lit|sky>, and the noise family's three additions:
    noise_unused_first (table 0 in LDS but unread), noise_shifted (hit points
    with negative x, y and z) and noise_general (tier 4)."""
    out = _parity(gpu, oracle, rt, capi, name)
    if name.startswith("ends_"):
        # Mix(lamp, L, 1.5) emits (1 - 1.5) * lamp: the reference has no clamp, nor has the kernel
        assert out["gpu"][0].min() < 0.0


@pytest.mark.parametrize("name", mw.FURNACE)
def test_furnace(gpu, oracle, rt, capi, name):
    """A sphere and a quad of the material in a uniform white environment:
    Transparent passes the ray on, SpherePDF's and CosinePDF's f / pdf is 1 at
    albedo 1, a white Dielectric attenuates by 1 -- every escaping path
    carries exactly 1, whatever the oracle says."""
    out = _parity(gpu, oracle, rt, capi, "furnace_" + name)
    np.testing.assert_allclose(out["gpu"][0], 1.0, rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", sorted(mw.EMISSION))
def test_emission(gpu, oracle, rt, capi, name):
    """One quad over the whole frame, black background, depth 1: nested is
    DiffuseLight((.25, .5, 1), DiffuseLight((.5, .25, .125))), the sum of the
    two colours (emitted_tree, tier 4); mix is Mix(DiffuseLight(c),
    DiffuseLight(c), .25), 0.75 c + 0.25 c = c exactly (the one-level
    shortcut of tiers 2 / 3)."""
    out = _parity(gpu, oracle, rt, capi, "emission_" + name)
    lin = out["gpu"][0]
    np.testing.assert_array_equal(lin, np.broadcast_to(np.float32(mw.EMISSION[name]), lin.shape))


def test_wrapper_depth_limit_render(gpu, rt, capi):
    """Five nested Mix levels: rt_render refuses the world as rt_world_info_get
    does (tests/test_materials_cpu.py); four render."""
    def world(levels):
        s = rt.Scene(gpu)
        w = s.Hittables()
        w.add(s.Sphere((0, 0, -2), 1.0, mw.nested_mix(s, levels)))
        cam = rt.Camera()
        cam.image_width = 8
        cam.samples_per_pixel = 1
        cam.background = s.SkyGradient()
        return w, cam
    w, cam = world(5)
    with pytest.raises(capi.RtError) as e:
        cam.render(w, None)
    assert e.value.code == -6  # RT_EUNSUPPORTED
    assert "4 levels" in str(e.value)
    w, cam = world(4)
    lin, _, st = cam.render(w, None)
    assert st.panics == 0 and np.isfinite(lin).all()
