"""The Disney BSDF on the GPU (kernel tier 5) against the test-side restatement
(tests/cpp/disney_oracle.cpp): the device functions bit for bit through
rt_disney_selftest, rtcr::pow_2m4 on the device against its host build, three
rendered worlds at test_parity_gpu's bars, and the hit / occlusion queries of
a Disney world against its Lambertian twin.

Measured on an MI355X: every self-test case bit-equal; the three frames
RMSE 0 with no diverged (pixel, s_i) sum and no panic on either side.
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
import disney_query as dq
from test_parity_gpu import check, gpu_partials

pytestmark = pytest.mark.gpu

SETS = list(dq.PARAM_SETS)


# ---------------------------------------------------------------- self-test
def _compare(gpu, fn, name, cases):
    g = dq.selftest(gpu, fn, name, cases)
    o = dq.selftest(dq.driver(), fn, name, cases, oracle=True)
    same = dq.same_bits(g, o)
    bad = np.flatnonzero(~same.all(axis=1))
    print(f"fn {fn} [{name}]: {len(cases)} cases, {len(bad)} differ, panics gpu {int(g[:, 5].sum())} / "
          f"oracle {int(o[:, 5].sum())}")
    if len(bad):
        i = bad[0]
        print("first:", list(cases[i]), "gpu", [x.hex() for x in g[i]], "oracle", [x.hex() for x in o[i]])
    assert len(bad) == 0, (name, fn, bad[:8])
    return g


@pytest.mark.parametrize("name", SETS)
def test_evaluate_disney_bits(gpu, name):
    """fn 0: 2 048 random unit-vector pairs and the hard cases, as u64 bit patterns."""
    cases = dq.eval_cases()
    g = _compare(gpu, 0, name, cases)
    assert g[:, 5].sum() >= 2  # the half-vector panic cases panic
    assert g[:2048, 5].sum() == 0


@pytest.mark.parametrize("name", SETS)
def test_generate_bits(gpu, name):
    """fn 1: 2 048 random (normal, v_out, draws), |n.x| > 0.9, the lobe-boundary draws."""
    cases = dq.gen_cases(name)
    g = _compare(gpu, 1, name, cases)
    some = g[:, 0] == 1.0
    assert some.sum() > 300
    n = np.linalg.norm(g[some, 1:4], axis=1)
    assert np.abs(n - 1.0).max() < 1e-12  # UnitVec3
    assert set(np.unique(g[g[:, 5] == 0.0, 4])) <= {1.0, 3.0, 4.0}  # lobe draw (+ r0, r1 (+ one more)); 1: None before any


def test_pow_2m4_device_equals_host(gpu, tmp_path):
    """rt_math_selftest fn 10 on the pow check's argument list = the host build of pow_2m4, bit for bit."""
    exe, dump = str(tmp_path / "pow_check"), str(tmp_path / "pow.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tests", "cpp", "pow_check.cpp"),
                    "-lquadmath", "-o", exe], check=True, timeout=300)
    r = json.loads(subprocess.run([exe, "60000", dump], check=True, capture_output=True, text=True, timeout=300).stdout)
    raw = np.fromfile(dump, dtype=np.float64)
    args, host = np.ascontiguousarray(raw[:r["n"]]), raw[r["n"]:]
    out = np.zeros_like(args)
    dp = C.POINTER(C.c_double)
    gpu.check(gpu.math_selftest(10, 0, args.ctypes.data_as(dp), None, out.ctypes.data_as(dp), len(args)))
    assert dq.same_bits(out, host).all()
    ocml = np.zeros_like(args)
    gpu.check(gpu.math_selftest(10, 1, args.ctypes.data_as(dp), None, ocml.ctypes.data_as(dp), len(args)))
    print(f"pow_2m4: {len(args)} arguments, device = host; ocml's pow differs on {int((~dq.same_bits(ocml, host)).sum())}")


# ---------------------------------------------------------------- renders
def _info(gpu, capi, s, world, lights, cam):
    info = capi.RtWorldInfo()
    bg = cam.background.h if cam.background is not None else -1
    gpu.check(gpu.world_info_get(s.s, world.h, -1 if lights is None else lights.h, bg, 0, C.byref(info)))
    return info


@pytest.mark.parametrize("name", list(dq.WORLDS))
def test_render_parity(gpu, rt, capi, name):
    """32 x 18, 16 spp, depth 8, seed 1 at check()'s default bars; kernel tier
    5; the same panic count (0) on both sides.  The project's stronger claim
    -- RMSE 0, no diverged (pixel, s_i) sum -- is printed (measured: 0 and 0
    on all three worlds)."""
    s = rt.Scene(gpu)
    world, lights, cam = dq.WORLDS[name](s)
    info = _info(gpu, capi, s, world, lights, cam)
    assert info.kernel_tier == 5 and info.features & dq.feature_bit("F_DISNEY")
    lin, srgb, st = cam.render(world, lights, seed=1)
    part = gpu_partials(gpu, s, cam, lin.shape[0])
    o_lin, o_srgb, o_part, o_panics = dq.reference(name)
    rmse = check({"gpu": (lin, srgb, part), "oracle": (o_lin, o_srgb, o_part)})
    diverged = np.flatnonzero(np.any(~dq.same_bits(part, o_part).reshape(-1, 3), axis=1))
    # (the kernel runs ray_color as a loop and the oracle as the recursion: equal paths agree to ~1e-15
    # relative, not to the bit; conftest.divergence counts the sums whose paths parted)
    print(f"{name}: panics gpu {st.panics} / oracle {o_panics}; (pixel, s_i) sums not bit-equal: {len(diverged)} of "
          f"{part.size // 3}")
    assert st.panics == o_panics == 0
    assert lin.max() > 0.05  # the frame shows something


# ---------------------------------------------------------------- queries
def test_queries_equal_the_lambertian_twin(gpu, rt):
    """rt_world_hit / rt_world_occluded on lobes_sky's world for 576 primary
    rays = the same calls on the world rebuilt with Lambertian in every Disney
    slot: record for record, mat included, byte for byte."""
    import hit_query as hq
    recs, occ = [], []
    for disney in (True, False):
        s = rt.Scene(gpu)
        world, _, cam = dq.world_lobes_sky(s, disney=disney)
        saved = (hq.GRID_W, hq.GRID_H)
        hq.GRID_W, hq.GRID_H = 32, 18
        try:
            rays = hq.grid_rays(cam)
        finally:
            hq.GRID_W, hq.GRID_H = saved
        assert len(rays) == 576
        recs.append(s.hit(world, rays))
        occ.append(s.occluded(world, rays))
        if disney:  # a render in between: the query's world and the render's are flattened apart
            lin, _, st = cam.render(world, None, seed=1)
            assert st.panics == 0
            recs.append(s.hit(world, rays))
            occ.append(s.occluded(world, rays))
    assert (recs[0]["flags"] & 1).sum() > 100 and occ[0].sum() == (recs[0]["flags"] & 1).sum()
    assert len(set(recs[0]["mat"][(recs[0]["flags"] & 1) != 0])) >= 7
    for r in recs[1:]:
        assert r.tobytes() == recs[0].tobytes()
    for o in occ[1:]:
        assert o.tobytes() == occ[0].tobytes()
