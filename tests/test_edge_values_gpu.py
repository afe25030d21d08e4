"""Edge values on the GPU: the Disney device functions, the path kernel and
the scatter / radiance queries at parameter sets where disney.rs is singular
or changes branch, and Texture::value at the addresses where texture.rs
rounds, clamps, wraps or casts -- against the oracle (and, for the textures,
the numpy model of tests/edge_query.py), bit for bit, NaN equal to NaN, no
record left out.  tests/test_edge_values_cpu.py holds the oracle-side half:
the closed forms, the reach of every edge class and model == oracle.
"""
import numpy as np
import pytest

import disney_query as dq
import edge_query as eq
import obj_disney_query as oq
import radiance_query as rq
import scatter_query as sq
from conftest import divergence
from test_parity_gpu import gpu_partials

pytestmark = pytest.mark.gpu


# ================================================================ A. Disney
def _selftest_equal(gpu, fn, name):
    cases = dq.eval_cases() if fn == 0 else eq.edge_gen_cases(name)
    for color, rgb in eq.EDGE_COLORS.items():
        g = dq.selftest(gpu, fn, eq.EDGE_SETS[name], cases, color=rgb)
        o = eq.oracle_selftest(fn, name, color)
        bad = np.flatnonzero(~dq.same_bits(g, o).all(axis=1))
        print(f"fn {fn} [{name}, {color}]: {len(cases)} cases, {len(bad)} differ, panics gpu {int(g[:, 5].sum())} / "
              f"oracle {int(o[:, 5].sum())}, non-finite rows {int((~np.isfinite(o)).any(axis=1).sum())}")
        if len(bad):
            i = bad[0]
            print("first:", list(cases[i]), "gpu", [x.hex() for x in g[i]], "oracle", [x.hex() for x in o[i]])
        assert len(bad) == 0, (name, color, fn, bad[:8])


@pytest.mark.parametrize("name", eq.EDGE_NAMES)
def test_evaluate_disney_bits_at_edges(gpu, name):
    """rt_disney_selftest fn 0 on eval_cases() at each edge set and the three
    base colours = orcx_disney_selftest in every output double."""
    _selftest_equal(gpu, 0, name)


@pytest.mark.parametrize("name", eq.EDGE_NAMES)
def test_generate_bits_at_edges(gpu, name):
    """fn 1 on the set's own cases (its lobe-boundary draws where its running sums are finite)."""
    _selftest_equal(gpu, 1, name)


def _scatter_equal(gpu, rt, k):
    rays, ev, want = eq.edge_scatter_reference(k)
    s = rt.Scene(gpu)
    world, _, cam = eq.edge_world(s, k)
    info = oq.world_info(gpu, s, world, None, cam.background)
    assert info.kernel_tier == 5
    got = s.scatter(world, None, rays, eval_dirs=ev, background=cam.background, seed=rq.SEED, vertex=1, sample=0)
    bad = eq.differing_fields(got, want)
    f = want["flags"]
    print(f"world {k}: {len(want)} records; oracle: hits {int((want['hit']['flags'] & 1).sum())}, PDF "
          f"{int(((f & sq.PDF) != 0).sum())}, NO_SAMPLE {int(((f & sq.NO_SAMPLE) != 0).sum())}, PANIC "
          f"{int(((f & sq.PANIC) != 0).sum())}; fields that differ: { {n: len(v) for n, v in bad.items()} }")
    if bad:
        sq.report(f"world {k}", got, want, bad)
    assert not bad, {n: len(v) for n, v in bad.items()}
    return s, world, cam, rays


@pytest.mark.parametrize("k", eq.RENDER_WORLDS)
def test_edge_world_render_and_scatter(gpu, rt, k):
    """Each edge world: rt_world_scatter on the frame's primary rays bit-equal
    in every field, the NO_SAMPLE and PANIC flags included; rt_render's f64
    (pixel, s_i) partial sums bit-equal to the oracle's.  The kernel gathers
    a path's radiance front to back (L += beta * e; beta *= (1 / pdf) * f),
    the reference back to front (e + (f * deeper) / pdf), and the two round
    differently in the last bits, so the sums are held bit-equal to the oracle
    run in the kernel's order (orcx_render_partials_loop,
    tests/cpp/edge_oracle.cpp: the same hits, draws and PDF values), with no
    sum diverged from the recursion's (conftest.divergence), the linear frame
    bit-equal to the recursion's, the sRGB bytes equal, no panic on either
    side."""
    s, world, cam, rays = _scatter_equal(gpu, rt, k)
    lin, srgb, st = cam.render(world, None, seed=1)
    part = gpu_partials(gpu, s, cam, lin.shape[0])
    o_lin, o_srgb, o_part, o_panics, o_loop = eq.edge_reference(k)
    not_loop = int(np.any(~dq.same_bits(part, o_loop).reshape(-1, 3), axis=1).sum())
    not_rec = int(np.any(~dq.same_bits(part, o_part).reshape(-1, 3), axis=1).sum())
    print(f"world {k}: panics gpu {st.panics} / oracle {o_panics}; (pixel, s_i) sums not bit-equal to the loop-order "
          f"oracle {not_loop}, to the recursion {not_rec}, of {part.size // 3}; diverged {divergence(part, o_part)}")
    assert not_loop == 0
    assert np.isfinite(part).all() and divergence(part, o_part) == 0.0
    assert dq.same_bits(lin, o_lin).all() and srgb.tobytes() == o_srgb.tobytes()
    assert int(st.panics) == o_panics == 0
    assert lin.max() > 0.05 and lin.std() > 0.01


def test_panic_world_returns_the_flag(gpu, rt):
    """The sets at which the reference panics (a NaN radiance, the exhausted
    conditions, the square root of a negative base colour): the scatter
    records carry RT_SCATTER_PANIC exactly where the oracle's do, every other
    field equal; rt_world_radiance at depth 8 and 4 samples a ray counts the
    oracle's panics and ray_color calls on every ray -- a path that carries a
    NaN pdf to the depth limit included, where the recursion's (f * BLACK) /
    NaN is the NaN camera.rs:323 asserts on; and rt_render completes and
    reports RT_EPANIC with the count, as the oracle's frame ends in RT_EPANIC:
    no fault, no hang."""
    k = eq.PANIC_WORLD
    s, world, cam, rays = _scatter_equal(gpu, rt, k)
    want = eq.edge_scatter_reference(k)[2]
    first = (want["flags"] & sq.PANIC) != 0
    assert first.sum() >= 20
    for samples in (1, 4):
        o_rgb, o_rays, o_panics = eq.edge_radiance_reference(k, samples)
        rgb, nrays, panics = s.radiance(world, None, rays, max_depth=dq.DEPTH, samples=samples, seed=rq.SEED,
                                        background=cam.background)
        print(f"panic world, {samples} sample(s): radiance panics gpu {int(panics.sum())} / oracle {int(o_panics.sum())}, "
              f"differing at {np.flatnonzero(panics != o_panics)}, rays differing at {np.flatnonzero(nrays != o_rays)}")
        assert np.array_equal(panics, o_panics) and np.array_equal(nrays, o_rays)
        assert (panics[first] >= 1).all() and np.isfinite(rgb).all()
        assert o_panics.sum() >= 20
    with pytest.raises(Exception, match="RT_EPANIC"):  # the frame: the panic count as an error, as the oracle's frame
        cam.render(world, None, seed=1)
    again = s.scatter(world, None, rays[:64], background=cam.background, seed=rq.SEED, vertex=1, sample=0)
    assert sq.same_bytes(again["hit"]["t"], want["hit"]["t"][:64])  # and the device goes on answering


# ---------------------------------------------------------------- the MTL spelling
@pytest.mark.parametrize("name", eq.mtl_sets())
def test_mtl_edge_values_equal_a_hand_built_twin(gpu, rt, name):
    """One triangle whose MTL carries an edge set's numbers, loaded with
    RT_OBJ_VANILLA | RT_OBJ_DISNEY (the flatten accepts every finite value),
    against the hand-built twin: 64 front-face rays, byte-equal records in
    every field a material decides.  With the vanilla flag the reference turns
    `Pm 1` into Metal and a Tf mean of 1 into Dielectric before it considers
    Disney, so the corner_01 / _10 / _11 and trans_ior_* spellings compare
    those materials (the twin follows), `Ni 1.0` reaches a Dielectric, not a
    Disney, and `thin`, flatness and the tints have no MTL spelling: 23 of the
    30 spellings carry their edge into a Disney material."""
    rays, ev = oq.tri_rays(64)
    idx = (np.arange(64, dtype=np.uint32) * 7919) % 100003
    for kd in (oq.TWIN_KD, eq.EDGE_COLORS["gamut"]):
        out = []
        for build in (eq.mtl_world_loaded, eq.mtl_world_twin):
            s = rt.Scene(gpu)
            world = build(s, name, kd)
            info = oq.world_info(gpu, s, world)  # the flatten: refuses nothing
            assert info.primitives == 1
            out.append(s.scatter(world, None, rays, eval_dirs=ev, indices=idx, seed=rq.SEED, vertex=2, sample=1))
        loaded, twin = out
        assert np.all(loaded["hit"]["flags"] == 3) and np.all(twin["hit"]["flags"] == 3)
        for k in ("emitted", "f", "pdf", "origin", "dir", "eval_f", "eval_pdf", "flags", "draws"):
            assert sq.same_bytes(loaded[k], twin[k]), (name, k)


# ================================================================ B. texture addressing and the casts
@pytest.mark.parametrize("tier", eq.TIERS)
def test_texture_probes_on_every_tier(gpu, rt, tier):
    """Every probe ray (image nearest / bilinear at 1x1, 1x5, 5x1 and 4x3 on
    quads and spheres, checkers whose `as i32` saturates either way, Perlin
    noise out to 2^62, the environment) through rt_world_scatter in a world
    that flattens to `tier`: every field of every record = the oracle's; the
    emitted colour = the numpy model's from the GPU's own (u, v, p) wherever
    a model exists (everything but the noise, and the environment off the
    axes); and rt_world_radiance at depth 1 returns the same colours (black
    and a counted panic where the colour is NaN)."""
    want, o_rgb, _ = eq.probe_reference()
    rays, n_obj = eq.probe_rays()
    s = rt.Scene(gpu)
    world, bg = eq.probe_world(s, tier)
    info = oq.world_info(gpu, s, world, None, bg)
    assert info.kernel_tier == tier
    got = s.scatter(world, None, rays, background=bg, seed=rq.SEED)
    bad = eq.differing_fields(got, want)
    per_group = {g["name"]: int((~dq.same_bits(got["emitted"][g["slice"]], want["emitted"][g["slice"]])).any(axis=1).sum())
                 for g in eq.probe_groups()}
    print(f"tier {tier}: {len(want)} records, fields that differ: { {k: len(v) for k, v in bad.items()} }; emitted "
          f"differing by group: { {k: v for k, v in per_group.items() if v} }")
    if bad:
        sq.report(f"tier {tier}", got, want, bad)
    assert not bad, {k: len(v) for k, v in bad.items()}
    modelled = 0
    for g in eq.probe_groups():
        if eq.has_noise(g["tex"]):
            continue
        h = got["hit"][g["slice"]]
        model = eq.model_value(g["tex"], h["u"], h["v"], h["p"])
        assert dq.same_bits(model, got["emitted"][g["slice"]]).all(), g["name"]
        modelled += len(h)
    u, v, p = eq.env_uv(rays[n_obj:n_obj + eq.AXIS_ENV, 3:6])
    assert dq.same_bits(eq.model_value(eq.ENV_TEX, u, v, p), got["emitted"][n_obj:n_obj + eq.AXIS_ENV]).all()
    # depth 1: the emission, or the background.  Where that is NaN (a bilinear lookup at a NaN v) the reference's
    # ray_color hands the NaN up (camera.rs:292-294) and so does the oracle; rt_world_radiance, as documented,
    # counts a NaN result as a panic and returns black
    rgb, _, panics = s.radiance(world, None, rays, max_depth=1, samples=1, seed=rq.SEED, background=bg)
    nan = np.isnan(o_rgb).any(axis=1)
    expect = np.where(nan[:, None], 0.0, o_rgb)
    print(f"tier {tier}: {modelled} records against the model; radiance not as expected "
          f"{int((~dq.same_bits(rgb, expect)).any(axis=1).sum())}, NaN emissions {int(nan.sum())}")
    assert nan.sum() >= 8 and np.array_equal(panics, nan.astype(np.uint32))
    assert dq.same_bits(rgb, expect).all()


def test_obj_constant_vt_triangles(gpu, rt):
    """Triangles whose three vt are one constant (-1e-20, the integers -2..2,
    2^52 + 0.5, -2^53, +-1e300, for u and for v), emitting through map_Ke, with
    and without Mix::from_image(Transparent, .., map_d): rt_world_scatter =
    the oracle in every field and = the model in the emitted colour (the texel
    identities of tests/test_edge_values_cpu.py), and the 16 x 9, 4 spp frame's
    partial sums are the oracle's bit for bit -- the path kernel's jittered
    rays land in the same classes."""
    want, o_part, o_lin, o_panics = eq.obj_reference()
    rays, tri = eq.obj_rays()
    s = rt.Scene(gpu)
    world, _, cam = eq.obj_world(s)
    info = oq.world_info(gpu, s, world, None, cam.background)
    assert info.kernel_tier == 5 and info.primitives == len(eq.obj_cases())
    got = s.scatter(world, None, rays, background=cam.background, seed=rq.SEED)
    bad = eq.differing_fields(got, want)
    if bad:
        sq.report("obj", got, want, bad)
    assert not bad, {k: len(v) for k, v in bad.items()}
    assert dq.same_bits(eq.obj_model(tri)[0], got["emitted"]).all()
    lin, _, st = cam.render(world, None, seed=1)
    part = gpu_partials(gpu, s, cam, lin.shape[0])
    diverged = int(np.any(~dq.same_bits(part, o_part).reshape(-1, 3), axis=1).sum())
    print(f"obj: {len(want)} records; frame panics gpu {st.panics} / oracle {o_panics}; (pixel, s_i) sums not bit-equal "
          f"{diverged} of {part.size // 3}")
    assert int(st.panics) == o_panics == 0 and diverged == 0 and dq.same_bits(lin, o_lin).all()
