"""Edge values without a GPU: the oracle side of tests/test_edge_values_gpu.py
run alone, the closed forms the edge sets have, the reach of every edge class,
and the numpy model of texture.rs (tests/edge_query.py) against the oracle, so
that an oracle defect shows here.

Every comparison is on bit patterns, NaN equal to NaN.
"""
import math

import numpy as np
import pytest

from conftest import divergence, pkg_module
import disney_query as dq
import edge_query as eq
import scatter_query as sq


# ================================================================ A. Disney
@pytest.mark.parametrize("name", eq.EDGE_NAMES)
def test_oracle_selftest_runs_at_every_edge_set(name):
    """orcx_disney_selftest fn 0 and fn 1 at each edge set and colour: it
    returns, a panicking row is zeros and the flag, and the generated
    directions are unit vectors."""
    for color in eq.EDGE_COLORS:
        e = eq.oracle_selftest(0, name, color)
        g = eq.oracle_selftest(1, name, color)
        for out in (e, g):
            assert set(np.unique(out[:, 5])) <= {0.0, 1.0}
            assert not out[out[:, 5] == 1.0, :5].any()
        some = (g[:, 0] == 1.0) & (g[:, 5] == 0.0)
        if some.any():
            n = np.linalg.norm(g[some, 1:4], axis=1)
            assert np.abs(n - 1.0).max() < 1e-12, (name, color)  # a sanity bound (UnitVec3), not a comparison
        print(f"{name} [{color}]: fn 0 panics {int(e[:, 5].sum())}, non-finite rows "
              f"{int((~np.isfinite(e[:, :5])).any(axis=1).sum())}; fn 1 panics {int(g[:, 5].sum())}, samples "
              f"{int(some.sum())}, draws {np.bincount(g[:, 4].astype(int)).tolist()}")


def test_reach_anisotropic_floor_and_nan_routes():
    """ax == 0.001 by the floor (roughness^2 / aspect below it) and by the NaN
    route (0/0, or sqrt of a negative): f64::max drops the NaN."""
    routes = {n: eq.aniso_params(p.get("roughness", 0.5), p.get("anisotropic", 0.0)) for n, p in eq.EDGE_SETS.items()}
    assert routes["rough_0"] == (0.001, 0.001, "floor")
    assert routes["rough_1e-3"] == (0.001, 0.001, "floor")
    assert routes["aniso_2"] == (0.001, 0.001, "nan")          # aspect = sqrt(-0.8)
    assert routes["aniso_10/9_rough_0"][2] == "nan"            # 0 / 0
    assert routes["aniso_10/9_rough_0"][:2] == (0.001, 0.001)
    # the floor itself and its neighbours: at least one side of it is the floor, one is not
    r = [routes[n][0] for n in ("rough_floor_lo", "rough_floor", "rough_floor_hi")]
    assert r[0] == 0.001 and r[2] > 0.001 and r[0] <= r[1] <= r[2]
    assert routes["aniso_1"][0] > routes["aniso_1"][1] and routes["aniso_-1"][0] < routes["aniso_-1"][1]


def test_reach_each_gtr1_branch():
    """gtr1's a >= 1 branch (1 / pi) at gloss -10; the logarithm branch at gloss 0, 1 and 1.5 (a < 0 there)."""
    a = {n: eq.gtr1_a(eq.EDGE_SETS[n]) for n in ("coat_gloss_0", "coat_gloss_1", "coat_gloss_1.5", "coat_gloss_-10")}
    assert a["coat_gloss_-10"] >= 1.0
    assert a["coat_gloss_0"] == 0.1 and a["coat_gloss_1"] == 0.001 and a["coat_gloss_1.5"] < 0.0
    # and the branch shows: at normal incidence (v_out = v_in = n) on a black base the reflectance is
    # (clearcoat + 0) + specular, the clearcoat value 0.25 * 1 * d * f * 1 * 1 with d = 1 / pi
    row = np.flatnonzero((dq.eval_cases()[:, :7] == [0, 1, 0, 0, 1, 0, 1]).all(axis=1))[0]
    coat = eq.oracle_selftest(0, "coat_gloss_-10", "black")[row]
    plain = eq.oracle_selftest(0, "coat_-1", "black")[row]
    f = 1.0 * (1.0 - 0.04) + 0.0 * 0.04  # schlick_f64(0.04, 1): lerp(1, schlick_weight(1) = 0, 0.04)
    want = 0.25 * 1.0 * (1.0 / math.pi) * f * 1.0 * 1.0
    assert coat[5] == plain[5] == 0.0 and (coat[:3] == want + plain[:3]).all(), (coat, plain, want)


def test_clearcoat_at_or_below_zero_is_no_lobe():
    """clearcoat <= 0: evaluate_clearcoat is (0, 0, 0) and the lobe's weight
    clamps to 0 -- every output double of clearcoat -1 equals the default's."""
    for color in eq.EDGE_COLORS:
        for fn in (0, 1):
            cases = dq.eval_cases() if fn == 0 else eq.edge_gen_cases("coat_-1")
            base = dq.selftest(eq.driver(), fn, {}, cases, oracle=True, color=eq.EDGE_COLORS[color])
            assert dq.same_bits(eq.oracle_selftest(fn, "coat_-1", color), base).all()
    assert dq.lobe_pdfs(dict(clearcoat=-1.0)) == dq.lobe_pdfs({})
    assert dq.lobe_pdfs(dict(clearcoat=2.0)) == dq.lobe_pdfs(dict(clearcoat=1.0))


def test_fresnel_is_zero_at_ior_one():
    """spec_trans 1, ior 1, front face, v_out = v_in = the normal: the
    dielectric Fresnel term is exactly 0, so the specular lobe adds nothing
    and the transmission lobe is c t (1 - 0) gl gv d colour with c = gl = gv
    = 1, t = 1 / 2^2 and d = 1 / (pi ax ay)."""
    row = np.flatnonzero((dq.eval_cases()[:, :7] == [0, 1, 0, 0, 1, 0, 1]).all(axis=1))[0]
    out = eq.oracle_selftest(0, "trans_ior_1", "grey")[row]
    ax, ay, _ = eq.aniso_params(0.5, 0.0)
    d = 1.0 / (math.pi * ax * ay * 1.0)
    want = 1.0 * 0.25 * (1.0 - 0.0) * 1.0 * 1.0 * d * 0.8
    assert out[5] == 0.0 and (out[:3] == want).all(), (out, want)


CORNERS = {"corner_00": (0.5, 0.5, 0.0, 0.0), "corner_10": (1.0, 0.0, 0.0, 0.0), "corner_01": (0.0, 0.0, 0.0, 1.0),
           "corner_11": (1.0, 0.0, 0.0, 0.0)}


@pytest.mark.parametrize("name", list(CORNERS))
def test_corner_lobe_probabilities(name):
    """(p_specular, p_diffuse, p_clearcoat, p_spec_trans) of a corner of
    (metallic, spec_trans) exactly; and generate() follows them: the specular
    sampler takes three draws, the diffuse and transmission samplers four (one,
    where the transmission sampler returns None before it draws)."""
    assert dq.lobe_pdfs(eq.EDGE_SETS[name]) == CORNERS[name]
    cases = eq.edge_gen_cases(name)
    out = eq.oracle_selftest(1, name, "grey")
    ok = out[:, 5] == 0.0
    p = cases[:, 7]
    if name in ("corner_10", "corner_11"):
        assert (out[ok, 4] == 3.0).all()
    elif name == "corner_01":
        assert (out[ok & (p > 0.0), 4] != 3.0).all() and (out[ok & (p == 0.0), 4] == 3.0).all()
        assert (p == 0.0).any() and set(np.unique(out[ok & (p > 0.0), 4])) <= {1.0, 4.0}
    else:
        assert (out[ok & (p <= 0.5), 4] == 3.0).all() and (out[ok & (p > 0.5), 4] == 4.0).all()
        assert (p == 0.5).any() and (p == eq.nxt(0.5)).any()


def test_zero_weight_sum_and_the_exhausted_panic():
    """metallic 2 / spec_trans 2: the weights sum to 0 and norm = 1/0; the
    probabilities are +-inf and NaN and generate() still picks a sampler.
    weights_nan: every probability is NaN and every generate() is the
    exhausted-conditions panic; evaluate_disney does not panic there."""
    ps, pd, pc, pt = dq.lobe_pdfs(eq.EDGE_SETS["metallic_2"])
    assert ps == math.inf and pd == -math.inf and math.isnan(pc) and math.isnan(pt)
    ps, pd, pc, pt = dq.lobe_pdfs(eq.EDGE_SETS["trans_2"])
    assert ps == -math.inf and pd == -math.inf and math.isnan(pc) and pt == math.inf
    assert all(math.isnan(x) for x in dq.lobe_pdfs(eq.EDGE_SETS["weights_nan"]))
    normalisable = np.linalg.norm(eq.edge_gen_cases("weights_nan")[:, 3:6], axis=1) > 0.0
    g = eq.oracle_selftest(1, "weights_nan", "grey")
    assert (g[normalisable, 5] == 1.0).all() and not g[:, :5].any()
    g2 = eq.oracle_selftest(1, "metallic_2", "grey")
    assert (g2[g2[:, 5] == 0.0, 4] == 3.0).all()   # p <= +inf: always the specular sampler
    g3 = eq.oracle_selftest(1, "trans_2", "grey")
    assert set(np.unique(g3[g3[:, 5] == 0.0, 4])) <= {1.0, 4.0}  # never p <= -inf or NaN: the transmission sampler
    e = eq.oracle_selftest(0, "weights_nan", "grey")
    assert e[:2048, 5].sum() == 0


def test_thin_out_of_gamut_panics():
    """thin with a negative base-colour channel: base_color.sqrt() is NaN, the
    reference's `The answer of sqrt is NaN!` -- the panic flag, on the rows that
    evaluate the transmission lobe."""
    e = eq.oracle_selftest(0, "thin_ior_1", "gamut")
    assert e[:2048, 5].sum() == 2048
    assert eq.oracle_selftest(0, "thin_ior_1", "grey")[:2048, 5].sum() == 0
    assert eq.oracle_selftest(0, "thin_flat_1", "gamut")[:2048, 5].sum() == 0  # no transmission weight: never evaluated


@pytest.mark.parametrize("k", range(eq.N_WORLDS))
def test_edge_worlds_on_the_oracle(k):
    """The oracle's frame and primary-ray scatter records of each edge world:
    every sphere is hit by some primary ray, and the records hold samples,
    NO_SAMPLE and PANIC flags to compare."""
    rays, ev, want = eq.edge_scatter_reference(k)
    hit = (want["hit"]["flags"] & 1) != 0
    f = want["flags"]
    rgb, nrays, rpanics = eq.edge_radiance_reference(k)
    print(f"world {k}: scatter: hits {int(hit.sum())}, materials {len(set(want['hit']['mat'][hit]))}, PDF "
          f"{int(((f & sq.PDF) != 0).sum())}, NO_SAMPLE {int(((f & sq.NO_SAMPLE) != 0).sum())}, PANIC "
          f"{int(((f & sq.PANIC) != 0).sum())}; radiance: rays that panicked {int((rpanics > 0).sum())}, non-finite "
          f"{int((~np.isfinite(rgb)).any(axis=1).sum())}")
    assert len(set(want["hit"]["mat"][hit])) == len(eq.world_members(k)) + 1  # every sphere and the ground
    assert ((f & sq.PDF) != 0).sum() >= 100
    if k in eq.RENDER_WORLDS:
        lin, _, part, panics, loop = eq.edge_reference(k)
        assert lin.shape == (18, 32, 3) and panics == 0 and lin.max() > 0.05
        # the same paths gathered in the kernel's order: finite, and no sum apart from the recursion's
        assert loop.shape == part.shape and np.isfinite(loop).all() and divergence(loop, part) == 0.0
    else:  # the reference's process ends at the first panic: so does the oracle's frame
        rt = pkg_module("raytracer")
        s = rt.Scene(eq.driver())
        world, lights, cam = eq.edge_world(s, k)
        with pytest.raises(Exception, match="RT_EPANIC"):
            cam.render(world, lights, seed=1)
        assert ((f & sq.PANIC) != 0).sum() >= 20 and (rpanics > 0).sum() >= 20


def test_every_set_stands_in_a_world():
    seen = {m for k in range(eq.N_WORLDS) for m in eq.world_members(k)}
    assert {n for n, _ in seen} == set(eq.EDGE_NAMES)
    assert all(len(eq.world_members(k)) <= 12 for k in range(eq.N_WORLDS))


# ================================================================ B. texture addressing and the casts
def _emitted_model(g, rec):
    h = rec["hit"]
    return eq.model_value(g["tex"], h["u"], h["v"], h["p"])


def _group(name):
    return next(g for g in eq.probe_groups() if g["name"] == name)


def test_probes_arrive_where_they_were_aimed():
    """Every quad probe hits its own quad at t = 1 with p = (x, y, z) exactly;
    every sphere probe hits its own sphere; every environment ray misses."""
    want, rgb, panics = eq.probe_reference()
    rays, n_obj = eq.probe_rays()
    assert panics.sum() == 0 and not (want["flags"] & sq.PANIC).any()
    assert ((want["hit"]["flags"][:n_obj] & 1) == 1).all() and (want["hit"]["flags"][n_obj:] == 0).all()
    for g in eq.probe_groups():
        h = want["hit"][g["slice"]]
        if g["kind"] == "quad":
            assert (h["t"] == 1.0).all() and (h["p"][:, 2] == g["z"]).all(), g["name"]
            assert (h["p"][:, :2] == g["rays"][:, :2]).all(), g["name"]
        else:
            d = np.linalg.norm(h["p"] - np.array(g["center"]), axis=1)
            # an aiming check, not a comparison: the hit lies on this group's sphere and on no other (100 apart)
            assert (np.abs(d - g["radius"]) <= 1e-9 * max(1.0, g["radius"])).all(), g["name"]
    # the radiance of depth 1 is the emission
    assert dq.same_bits(rgb, want["emitted"]).all()


def test_unit_quad_hands_the_texture_its_coordinates():
    """Q = 0, u = x, v = y: rec.u = x and rec.v = y exactly, the denormal and 1 - 2^-53 included."""
    want, _, _ = eq.probe_reference()
    for g in eq.probe_groups():
        if g["name"].startswith("image_"):
            h = want["hit"][g["slice"]]
            assert (sq.bits(h["u"]) == sq.bits(g["rays"][:, 0])).all()
            assert (sq.bits(h["v"]) == sq.bits(g["rays"][:, 1])).all()


@pytest.mark.parametrize("name", [g["name"] for g in eq.probe_groups() if not eq.has_noise(g["tex"])])
def test_model_equals_oracle(name):
    """The numpy model of texture.rs with Rust's casts written out = the
    oracle's emitted colour, bit for bit, from the oracle's own (u, v, p)."""
    want, _, _ = eq.probe_reference()
    g = _group(name)
    rec = want[g["slice"]]
    model = _emitted_model(g, rec)
    bad = np.flatnonzero(~dq.same_bits(model, rec["emitted"]).all(axis=1))
    if len(bad):
        i = bad[0]
        print(f"{name}: {len(bad)} of {len(rec)} differ; first: u {rec['hit']['u'][i]!r} v {rec['hit']['v'][i]!r} p "
              f"{rec['hit']['p'][i]} model {model[i]} oracle {rec['emitted'][i]}")
    assert len(bad) == 0, (name, len(bad), len(rec))


def test_reach_image_classes():
    """From the oracle's records: index == h, bilinear dx < 0 and dy < 0, x1 ==
    x0 (a 1-wide image, and the last column), u == 0.0, u == 1.0, v NaN.  The
    NaN v is the one way `as u32` leaves its range here (NaN -> 0): its
    argument is abs_fract times a size, or a floor already raised to 0, so it
    is never negative and never reaches 2^32."""
    want, _, _ = eq.probe_reference()
    seen = dict(j_eq_h=0, dx_neg=0, dy_neg=0, x1_eq_x0_last=0, x1_eq_x0_single=0, u0=0, u1=0, v_nan=0, sphere_u0=0,
                sphere_u1=0, denormal=0)
    for g in eq.probe_groups():
        if g["tex"][0] != "image":
            continue
        h = want["hit"][g["slice"]]
        (wd, ht), linear = g["tex"][1], g["tex"][2]
        _, m = eq.image_lookup(eq.image_texels(wd, ht), linear, h["u"], h["v"])
        seen["u0"] += int((h["u"] == 0.0).sum())
        seen["u1"] += int((h["u"] == 1.0).sum())
        seen["denormal"] += int((h["u"] == 5e-324).sum())
        seen["v_nan"] += int(np.isnan(h["v"]).sum())
        if g["kind"] == "sphere":
            seen["sphere_u0"] += int((h["u"] == 0.0).sum())
            seen["sphere_u1"] += int((h["u"] == 1.0).sum())
        if not linear:
            seen["j_eq_h"] += int((m["j"] == ht).sum())
        else:
            seen["dx_neg"] += int((m["dx"] < 0).sum())
            seen["dy_neg"] += int((m["dy"] < 0).sum())
            if wd == 1:
                seen["x1_eq_x0_single"] += int((m["x1"] == m["x0"]).sum())
            else:
                seen["x1_eq_x0_last"] += int(((m["x1"] == m["x0"]) & (m["x0"] == wd - 1)).sum())
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_reach_checker_casts():
    """Each side of `as i32`: a cell that saturates at i32::MAX, one at
    i32::MIN, the last cells before either, a sum that wraps, and negative
    odd and even cells next to 0."""
    want, _, _ = eq.probe_reference()
    seen = dict(sat_hi=0, sat_lo=0, max_exact=0, min_exact=0, wraps=0, neg_odd=0, neg_even=0, odd_by_saturation=0)
    for g in eq.probe_groups():
        if g["tex"][0] != "checker" or g["name"] == "checker_nested":
            continue
        p = want["hit"]["p"][g["slice"]]
        inv = 1.0 / g["tex"][1]
        with np.errstate(all="ignore"):
            raw = np.floor(inv * p)
        c = eq.checker_cells(g["tex"][1], p)
        seen["sat_hi"] += int((raw >= 2.0 ** 31).sum())
        seen["sat_lo"] += int((raw < -2.0 ** 31).sum())
        seen["max_exact"] += int((raw == 2.0 ** 31 - 1).sum())
        seen["min_exact"] += int((raw == -2.0 ** 31).sum())
        total = c.sum(axis=1)
        seen["wraps"] += int((total != eq.wrap_i32(total)).sum())
        seen["neg_odd"] += int(((c[:, 0] < 0) & (c[:, 0] > -4) & (c[:, 0] % 2 == 1)).sum())
        seen["neg_even"] += int(((c[:, 0] < 0) & (c[:, 0] > -4) & (c[:, 0] % 2 == 0)).sum())
        # a cell that is odd only because it saturated at i32::MAX, the other two even: INT_MIN there reads even
        sat = (raw >= 2.0 ** 31)
        seen["odd_by_saturation"] += int(((sat.sum(axis=1) == 1) & ((c % 2 == 1).sum(axis=1) == 1)).sum())
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_reach_perlin_cast():
    """`as i64` (perlin.rs:41): the probes reach coordinates whose later
    turbulence octaves (p doubled six times) pass +-2^63, both sides, and
    coordinates that stay inside."""
    want, _, _ = eq.probe_reference()
    hi = lo = inside = 0
    for g in eq.probe_groups():
        if g["tex"][0] != "noise":
            continue
        p = want["hit"]["p"][g["slice"]]
        top = p * 64.0
        hi += int((top >= 2.0 ** 63).any(axis=1).sum())
        lo += int((top <= -2.0 ** 63).any(axis=1).sum())
        inside += int((np.abs(top) < 2.0 ** 63).all(axis=1).sum())
        assert (eq.as_i64(top[top >= 2.0 ** 63]) == np.iinfo(np.int64).max).all()
    assert hi > 0 and lo > 0 and inside > 100


def test_environment_model_at_the_axes():
    """Environment::value's own (u, v): phi = pi - atan2(-z, x), unlike the
    sphere's.  At the six axis directions (any length) every libm argument is
    a signed zero or +-1 and the model's (u, v) is exact: model == oracle."""
    want, _, _ = eq.probe_reference()
    rays, n_obj = eq.probe_rays()
    env = want[n_obj:]
    d = rays[n_obj:n_obj + eq.AXIS_ENV, 3:6]
    u, v, p = eq.env_uv(d)
    model = eq.model_value(eq.ENV_TEX, u, v, p)
    assert dq.same_bits(model, env["emitted"][:eq.AXIS_ENV]).all()
    assert len({tuple(x) for x in env["emitted"]}) >= 8  # the lookup moves over the image
    assert not (env["flags"] & sq.PANIC).any() and np.isfinite(env["emitted"]).all()
    # reach: the environment's seam (x < 0) and both poles were read.  On the seam itself, z = +-0, u is exactly
    # 1.0 or 0.0 and abs_fract wraps both to column 0: one colour a height.  2^-30 off it the two sides read the
    # last column and the first (blended past the border, dx < 0): no colour in common.
    dirs = rays[n_obj:, 3:6]
    neg_x = dirs[:, 0] < 0.0
    on = neg_x & (dirs[:, 2] == 0.0)
    off = neg_x & (np.abs(dirs[:, 2]) == 2.0 ** -30 * np.abs(dirs[:, 0]))
    side = np.signbit(dirs[:, 2])
    colours = lambda m: {tuple(x) for x in env["emitted"][m]}
    assert (on & side).sum() >= 9 and (on & ~side).sum() >= 9 and colours(on & side) == colours(on & ~side)
    assert (off & side).sum() >= 9 and (off & ~side).sum() >= 9 and not (colours(off & side) & colours(off & ~side))
    # the poles themselves: v is exactly 1.0 (up) or 0.0 (down), and both wrap to row index h, clamped: the same
    # colours (as they are 2^-30 off the axis, where y still rounds to +-1); 2^-20 off it the two poles read opposite rows
    axis = (dirs[:, 0] == 0.0) & (dirs[:, 2] == 0.0)
    near = (np.abs(dirs[:, 0]) == 2.0 ** -20 * np.abs(dirs[:, 1])) & (dirs[:, 2] == 0.0)
    up = dirs[:, 1] > 0.0
    assert (axis & up).sum() >= 3 and (axis & ~up).sum() >= 3 and colours(axis & up) == colours(axis & ~up)
    assert (near & up).sum() >= 3 and (near & ~up).sum() >= 3 and not (colours(near & up) & colours(near & ~up))


# ---------------------------------------------------------------- OBJ triangles with constant vt
def test_obj_constant_vt_reads_the_expected_texel():
    """Every ray on a triangle whose three vt are one constant reads the texel
    the constant names, in closed form -- abs_fract(-1e-20) == 1.0 reads
    column w - 1 (index == w, clamped), an integer v reads row h - 1 (index ==
    h), 2^52 + 0.5, -2^53 and +-1e300 read texel column 0 -- and model ==
    oracle in every emitted double, with and without the map_d veil."""
    want, part, lin, panics = eq.obj_reference()
    rays, tri = eq.obj_rays()
    assert panics == 0 and (want["hit"]["flags"] == 3).all() and not (want["flags"] & sq.PANIC).any()
    assert (want["hit"]["t"] == 1.0).all()
    model, m = eq.obj_model(tri)
    assert dq.same_bits(model, want["emitted"]).all()
    ke, al = eq.obj_texels()
    cases = eq.obj_cases()
    for t, (cu, cv, veil) in enumerate(cases):
        col, row = eq.obj_expected_texel(cu, cv)
        e = want["emitted"][tri == t]
        expect = ke[row, col, :3].astype(float) * (al[row, col, 3] if veil else 1.0)
        assert (e == expect).all(), (cu, cv, veil, e[0], expect)
    # reach: abs_fract == 1.0, index == w, index == h
    assert (m["uu"] == 1.0).sum() >= 6 and (m["i"] == eq.OBJ_W).sum() >= 6 and (m["j"] == eq.OBJ_H).sum() >= 6
    assert ((m["uu"] == 0.0) & (np.abs([cases[t][0] for t in tri]) >= 1e300)).sum() >= 12  # a vt of +-1e300
    assert lin.shape == (9, 16, 3) and len({tuple(px) for px in lin.reshape(-1, 3)}) > 10  # the triangles show


# ---------------------------------------------------------------- the MTL spelling of the edge sets
@pytest.mark.parametrize("name", eq.mtl_sets())
def test_mtl_edge_values_load_and_equal_the_twin_on_the_oracle(product, rt, name):
    """An MTL that carries an edge set's numbers (`Pr 0`, `Ni 1.0`, `aniso 2`,
    `Pcr -10`, `Pm 2`, ...) loads with RT_OBJ_VANILLA | RT_OBJ_DISNEY and the
    product's flatten accepts it -- every value is finite, none is refused --
    and on the oracle its scatter records are byte-equal to the hand-built
    twin's."""
    import obj_disney_query as oq
    import radiance_query as rq
    rays, ev = oq.tri_rays(64)
    idx = (np.arange(64, dtype=np.uint32) * 7919) % 100003
    drv = eq.driver()
    for kd in (oq.TWIN_KD, eq.EDGE_COLORS["gamut"]):
        s = rt.Scene(product)
        assert oq.world_info(product, s, eq.mtl_world_loaded(s, name, kd)).primitives == 1
        out = []
        for build in (eq.mtl_world_loaded, eq.mtl_world_twin):
            s = rt.Scene(drv)
            world = build(s, name, kd)
            out.append(sq.oracle_scatter(drv, s, world, rays, eval_dirs=ev, indices=idx, seed=rq.SEED, vertex=2, sample=1))
        for k in ("emitted", "f", "pdf", "origin", "dir", "eval_f", "eval_pdf", "flags", "draws"):
            assert sq.same_bytes(out[0][k], out[1][k]), (name, k)
        assert (out[0]["hit"]["flags"] == 3).all()
