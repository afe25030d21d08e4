"""rt_world_occluded on the GPU: out[i] is the RT_HIT_FOUND bit of the record
the oracle's Hittable::hit driver returns for ray i (tests/hit_query.py), on
every ray of every world's set, on the product and on the check build.

The any-hit walk ends at the first accepted hit, so what can go wrong is what
a lane carries over from a walk that was dropped where it stood: words on its
stack, spheres in its queue, media in its queue.  Hence the whole sets (a fifth
to a half occluded, so every wave mixes dropped and finished walks), prefixes
around a wave's size, a query of more rays than the device holds lanes, where
every lane takes a further ray after a dropped walk, and queries interleaved
with hit queries and renders on one scene, which share the slot's stack
overflow buffer.
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
PAD = 256


@pytest.fixture(scope="module")
def builds(capi, gpu):
    # the check build is a build product (__graft_entry__.build() makes it): absent is a failure
    assert os.path.exists(CHECK_SO), "check build absent: make -C raytracer-2025_amd check (__graft_entry__.build())"
    chk = capi.Api(ctypes.CDLL(CHECK_SO), "rt_")
    assert not chk.missing, chk.missing
    return {"product": gpu, "check": chk}


def _found(rec):
    return ((rec["flags"] & hq.FOUND) != 0).astype(np.uint8)


def _upload(rays):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(-1).copy()).cuda()


def _device_query(scene, world, rays, flags, seed=SEED):
    """rt_world_occluded_device through torch's allocations on the current
    device; the PAD bytes past out[n] must come back as they were."""
    import torch
    n = len(rays)
    d_rays = _upload(rays)
    d_out = torch.full((n + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    scene.occluded_device(world, d_rays.data_ptr(), n, d_out.data_ptr(), seed=seed, flags=flags, stream=None)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    assert np.all(out[n:] == 0xA5), "bytes past out[n] were written"
    return out[:n]


def _report(name, rays, got, want, where=None):
    bad = np.nonzero(got != want)[0]
    print(f"{name}: {len(rays)} rays, {want.mean():.3f} occluded, {len(bad)} bytes differ from the driver"
          + "".join(f"\n  ray {i} {rays[i]}: gpu {got[i]} driver {want[i]}" for i in bad[:5]))
    for part, sl in (where or {}).items():
        nb = int((got[sl] != want[sl]).sum())
        if nb:
            print(f"  {part}: {nb} of {sl.stop - sl.start} differ")


@pytest.mark.parametrize("build", ["product", "check"])
@pytest.mark.parametrize("name", sorted(hq.WORLDS))
def test_world_occluded_equals_the_oracle(builds, capi, name, build):
    api = builds[build]
    _, flags, tier, _, _ = hq.WORLDS[name]
    rays, where, ref = hq.reference(name, SEED)
    want = _found(ref)
    s, w, cam, extras, _, _ = hq.world_case(api, name, tempfile.mkdtemp(prefix="hit_world_"))
    info = capi.RtWorldInfo()
    api.check(api.world_info_get(s.s, w.h, -1, -1, flags, ctypes.byref(info)))
    assert info.kernel_tier == tier
    got = s.occluded(w, rays, seed=SEED, flags=flags)
    assert got.dtype == np.uint8 and got.shape == (len(rays),)
    _report(f"{name} / {build} (tier {info.kernel_tier})", rays, got, want, where)
    assert np.all(got <= 1)
    assert np.array_equal(got, want)
    # the GPU's own records
    assert np.array_equal(got, _found(s.hit(w, rays, seed=SEED, flags=flags)))
    # a second call, and the device variant
    assert np.array_equal(s.occluded(w, rays, seed=SEED, flags=flags), got)
    assert np.array_equal(_device_query(s, w, rays, flags), got)
    # prefixes: a ray's answer and its medium draw are keyed by its index alone
    for n in (1, 63, 64, 65, 1025):
        assert len(rays) > n
        assert np.array_equal(s.occluded(w, rays[:n], seed=SEED, flags=flags), got[:n]), n
    # the device variant's own tail: a last wave with one ray in it
    assert np.array_equal(_device_query(s, w, rays[:65], flags), got[:65])


def test_the_seed_keys_the_medium_draw(builds):
    name = "cornell_smoke"
    seed = 0x1234567890ABCDEF
    rays, _, ref0 = hq.reference(name, SEED)
    drv = hq.driver(True)
    so, wo, _, _, _, _ = hq.world_case(drv, name, tempfile.mkdtemp(prefix="hit_world_"))
    want = _found(hq.oracle_hit(drv, so, wo, rays, seed=seed))
    assert np.any(want != _found(ref0))
    s, w, _, _, flags, _ = hq.world_case(builds["product"], name, tempfile.mkdtemp(prefix="hit_world_"))
    got = s.occluded(w, rays, seed=seed, flags=flags)
    _report(f"{name} at seed {seed:#x}", rays, got, want)
    assert np.array_equal(got, want)
    assert np.any(got != s.occluded(w, rays, seed=SEED, flags=flags))


@pytest.mark.parametrize("name", ["wide", "mesh", "cornell_smoke", "final_reduced"])
def test_more_rays_than_the_device_holds_lanes(builds, name):
    """600 000 rays drawn from all parts of the set, so that every wave mixes
    them: more than 256 CUs x 2 048 lanes, so lanes take a further ray after a
    walk that ended early with words on its stack and spheres or media queued.
    The driver is asked again for this very array (a medium's draw is keyed by
    the ray's index)."""
    n = 600_000
    small, _, _ = hq.reference(name, SEED)
    rays = np.ascontiguousarray(small[np.random.default_rng(7).integers(0, len(small), n)])
    drv = hq.driver(True)
    so, wo, _, _, _, _ = hq.world_case(drv, name, tempfile.mkdtemp(prefix="hit_world_"))
    want = _found(hq.oracle_hit(drv, so, wo, rays, seed=SEED))
    s, w, _, _, flags, _ = hq.world_case(builds["product"], name, tempfile.mkdtemp(prefix="hit_world_"))
    got = _device_query(s, w, rays, flags)
    _report(name, rays, got, want)
    assert np.all(got <= 1)
    assert np.array_equal(got, want)


def test_queries_interleaved_on_one_scene(builds, rt):
    """hit, occluded, hit, occluded of one world back to back on one stream,
    one synchronise at the end: the answers of the calls made alone (they
    share the scene's slot and its stack overflow buffer)."""
    import torch
    name = "final_reduced"
    rays, _, _ = hq.reference(name, SEED)
    n = len(rays)
    s, w, _, _, flags, _ = hq.world_case(builds["product"], name, tempfile.mkdtemp(prefix="hit_world_"))
    alone_rec = s.hit(w, rays, seed=SEED, flags=flags)
    alone_occ = s.occluded(w, rays, seed=SEED, flags=flags)
    assert np.array_equal(alone_occ, _found(alone_rec))
    d_rays = _upload(rays)
    recs = [torch.full((n * 80 + PAD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    occs = [torch.full((n + PAD,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    for k in range(2):
        s.hit_device(w, d_rays.data_ptr(), n, recs[k].data_ptr(), seed=SEED, flags=flags, stream=stream.cuda_stream)
        s.occluded_device(w, d_rays.data_ptr(), n, occs[k].data_ptr(), seed=SEED, flags=flags,
                          stream=stream.cuda_stream)
    stream.synchronize()
    for k in range(2):
        r, o = recs[k].cpu().numpy(), occs[k].cpu().numpy()
        assert np.all(r[n * 80:] == 0xA5) and np.all(o[n:] == 0xA5)
        assert r[:n * 80].tobytes() == alone_rec.tobytes(), k
        assert np.array_equal(o[:n], alone_occ), k


@pytest.mark.parametrize("build", ["product", "check"])
def test_renders_around_a_query_keep_the_golden_frame(builds, rt, build):
    """A render, an occlusion query of the same scene's world (another
    flattening: no lights, no background) and the render again: both frames
    are the committed golden one, and the queries around them the driver's."""
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
    got = scene.occluded(world, rays[:2304], seed=SEED)
    after, _, _ = cam.render(world, lights, seed=seed, row_offset=off, row_stride=stride)
    again = scene.occluded(world, rays[:2304], seed=SEED)
    assert np.array_equal(before, golden) and np.array_equal(after, golden)
    assert np.array_equal(got, _found(ref[:2304]))
    assert np.array_equal(again, got)
