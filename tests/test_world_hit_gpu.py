"""rt_world_hit on the GPU against the oracle's Hittable::hit, ray by ray.

Every world of tests/hit_query.py (basic tier: the worlds of
test_walk_rounds_gpu.py; a ~2 500-sphere world past the basic tier's LDS node
copy; mesh tier: a box and loose triangles under a BVH, and the reference's
mc.obj; full-flat tier: cornell_smoke; full tier: a reduced final scene) is
queried with its whole ray set -- a 64x36 pinhole grid, second-generation rays
that start on a surface, rays from inside spheres and boxes, axis-parallel
rays, directions scaled by 1e-3 and 1e3, other ray times, and t_max at half,
at, and one ulp under every first hit (tests/test_world_hit_cpu.py holds the
sets to that on the oracle alone) -- on the product and on the check build.

On every ray, none left out: flags, t, p, normal, u and v are bit-equal to
the driver's (the raw bytes compared), mat is equal wherever the driver names
one, the host and the device variant give the same bytes, a second call gives
the same bytes, and prefixes of 1, 63, 65 and 1025 rays give the prefix of
the whole set's answer (a ray's medium draw is keyed by its index alone), a
prefix of 65 through the device variant too, which writes no record past n.
"""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import hit_query as hq

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK_SO = os.path.join(ROOT, "raytracer-2025_amd", "librt_mi355x_check.so")
SEED = 0


@pytest.fixture(scope="module")
def builds(capi, gpu):
    # the check build is a build product (__graft_entry__.build() makes it): absent is a failure
    assert os.path.exists(CHECK_SO), "check build absent: make -C raytracer-2025_amd check (__graft_entry__.build())"
    chk = capi.Api(ctypes.CDLL(CHECK_SO), "rt_")
    assert not chk.missing, chk.missing
    return {"product": gpu, "check": chk}


def _device_query(scene, world, rays, flags):
    """rt_world_hit_device through torch's allocations on the current device."""
    import torch
    rt = hq.pkg_module("raytracer")
    n = len(rays)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()
    # (a wave's worth of records past the n-th: the lanes past n write nothing)
    d_out = torch.full(((n + 64) * 80,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.hit_device(world, d_rays.data_ptr(), n, d_out.data_ptr(), seed=SEED, flags=flags, stream=None)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[n * 80:] == 0xA5)
    return out[:n * 80].view(rt.HIT_DTYPE)


@pytest.mark.parametrize("build", ["product", "check"])
@pytest.mark.parametrize("name", sorted(hq.WORLDS))
def test_world_hit_equals_the_oracle(builds, capi, name, build):
    api = builds[build]
    _, flags, tier, _, _ = hq.WORLDS[name]
    rays, where, ref = hq.reference(name, SEED)
    s, w, cam, extras, _, _ = hq.world_case(api, name, tempfile.mkdtemp(prefix="hit_world_"))
    info = capi.RtWorldInfo()
    api.check(api.world_info_get(s.s, w.h, -1, -1, flags, ctypes.byref(info)))
    assert info.kernel_tier == tier
    got = s.hit(w, rays, seed=SEED, flags=flags)
    gb, rb = hq.geometry_bytes(got), hq.geometry_bytes(ref)
    bad = np.nonzero(np.any(gb != rb, axis=1))[0]
    print(f"{name} / {build}: {len(rays)} rays, tier {info.kernel_tier}, {len(bad)} records differ from the driver"
          + "".join(f"\n  ray {i} {rays[i]}:\n    gpu    {got[i]}\n    driver {ref[i]}" for i in bad[:5]))
    for part, sl in where.items():
        nb = int(np.any(gb[sl] != rb[sl], axis=1).sum())
        if nb:
            print(f"  {part}: {nb} of {sl.stop - sl.start} differ")
    assert np.array_equal(gb, rb)
    named = ref["mat"] >= 0
    assert np.array_equal(got["mat"][named], ref["mat"][named])
    assert np.all(got["mat"][(ref["flags"] & hq.FOUND) == 0] == -1)
    whole = got.tobytes()
    assert s.hit(w, rays, seed=SEED, flags=flags).tobytes() == whole
    assert _device_query(s, w, rays, flags).tobytes() == whole
    for n in (1, 63, 65, 1025):
        assert len(rays) > n
        assert s.hit(w, rays[:n], seed=SEED, flags=flags).tobytes() == got[:n].tobytes(), n
    # the device variant's own tail: a last wave with one ray in it, a grid of two waves
    assert _device_query(s, w, rays[:65], flags).tobytes() == got[:65].tobytes()


def test_the_seed_keys_the_medium_draw(builds, rt):
    """Another seed: other medium hits, the same surface hits, and still the driver's records."""
    name = "cornell_smoke"
    rays, where, ref0 = hq.reference(name, SEED)
    drv = hq.driver(True)
    so, wo, _, _, _, _ = hq.world_case(drv, name, tempfile.mkdtemp(prefix="hit_world_"))
    ref = hq.oracle_hit(drv, so, wo, rays, seed=0x1234567890ABCDEF)
    assert np.any(ref["flags"] != ref0["flags"])
    s, w, _, _, flags, _ = hq.world_case(builds["product"], name, tempfile.mkdtemp(prefix="hit_world_"))
    got = s.hit(w, rays, seed=0x1234567890ABCDEF, flags=flags)
    assert np.array_equal(hq.geometry_bytes(got), hq.geometry_bytes(ref))


@pytest.mark.parametrize("build", ["product", "check"])
def test_renders_around_a_query_keep_the_golden_frame(builds, rt, build):
    """A render, a query of the same scene's world (another flattening: no
    lights, no background) and the render again: both frames are the committed
    golden one (tests/golden/c3_48x48_s16_seed7.npy, as test_parity_gpu.py reads
    it), and the query between them is the driver's."""
    import importlib
    import sys
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    gen_golden = importlib.import_module("gen_golden")
    gname = "c3_48x48_s16_seed7"
    make, seed, off, stride = gen_golden.case(gname)
    golden = np.load(os.path.join(ROOT, "tests", "golden", gname + ".npy")).astype(np.float32)
    api = builds[build]
    scene = rt.Scene(api)
    world, lights, cam = make(scene)
    rays, _, ref = hq.reference("cornell_smoke", SEED)  # the same world
    before, _, _ = cam.render(world, lights, seed=seed, row_offset=off, row_stride=stride)
    got = scene.hit(world, rays[:2304], seed=SEED)
    after, _, _ = cam.render(world, lights, seed=seed, row_offset=off, row_stride=stride)
    again = scene.hit(world, rays[:2304], seed=SEED)
    assert np.array_equal(before, golden) and np.array_equal(after, golden)
    assert np.array_equal(hq.geometry_bytes(got), hq.geometry_bytes(ref[:2304]))
    assert got.tobytes() == again.tobytes()
